"""TEST INFRASTRUCTURE ONLY (checker, never shipped or measured): numpy float64 restatement of the
sklearn 1.7.2 cluster-quality metrics the reference calls:

  silhouette_samples / silhouette_score  sklearn/metrics/cluster/_unsupervised.py (silhouette_samples,
      _silhouette_reduce): per-row sums of euclidean distances by cluster, a = intra / (n_l - 1),
      b = min over other clusters of mean distance, s = (b - a) / max(a, b), 0 for singletons; mean.
      Called at src/Convolutional_VAE.py:320,337,361,399, src/Conditional_VAE.py:298, src/Simple_VAE.py:247.
  davies_bouldin_score     (_unsupervised.py davies_bouldin_score) src/Convolutional_VAE.py:400
  calinski_harabasz_score  (_unsupervised.py calinski_harabasz_score) src/Simple_VAE.py:257,263

Pinned: tests/test_oracle_cpu.py checks it against the committed sklearn outputs (tests/golden/metrics_*.npz,
made by tests/golden/make_golden.py with sklearn itself).
"""
from __future__ import annotations

import numpy as np

from .scaler_oracle import sums_exact


def _encode(labels):
    classes, enc = np.unique(np.asarray(labels), return_inverse=True)
    return enc.reshape(-1), len(classes)


def silhouette_sums(X, labels, chunk=512):
    """S[i][c] = sum over rows j of cluster c of ||x_i - x_j||, by direct differences of the float32 inputs in
    float64 (no Gram form: nothing cancels on data far from the origin)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    lab, k = _encode(labels)
    n, d = X.shape
    onehot = np.zeros((n, k))
    onehot[np.arange(n), lab] = 1.0
    S = np.empty((n, k))
    for i0 in range(0, n, chunk):
        xi = X[i0:i0 + chunk]
        d2 = np.zeros((xi.shape[0], n))
        for c in range(d):
            d2 += (xi[:, c, None] - X[None, :, c]) ** 2
        S[i0:i0 + chunk] = np.sqrt(d2) @ onehot
    return S


def silhouette_from_sums(S, labels):
    """sklearn's _silhouette_reduce + silhouette_samples finish: a = S[i][l_i] / (n_l - 1), b = min over the other
    clusters of S[i][c] / n_c, s = (b - a) / max(a, b); singleton clusters and max(a, b) == 0 give 0."""
    S = np.asarray(S, dtype=np.float64)
    lab, k = _encode(labels)
    n = S.shape[0]
    freqs = np.bincount(lab, minlength=k)
    intra = S[np.arange(n), lab]
    Sm = S / freqs[None, :]
    Sm[np.arange(n), lab] = np.inf
    inter = Sm.min(1)
    denom = (freqs - 1)[lab]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = intra / denom
        s = (inter - a) / np.maximum(a, inter)
    return np.nan_to_num(s)


def silhouette_samples(X, labels):
    return silhouette_from_sums(silhouette_sums(X, labels), labels)


def _sil_eps(d):
    # per pair, float32 unit roundoff u = 2^-24: one rounding in each difference -> 2u relative on its square; d fma
    # roundings on a sum of non-negative terms -> d u; the square root halves the relative error ((2 + d) / 2 u);
    # 2u on top for sqrtf and the float -> double conversion.  The float64 accumulation is below 2^-40 of that.
    return (d / 2.0 + 3.0) * 2.0 ** -24


def sums_bound(S, d):
    """|S_kernel - S| <= (d / 2 + 3) 2^-24 S for float32 direct-difference distances summed in float64."""
    return _sil_eps(d) * np.asarray(S, dtype=np.float64)


def samples_bound(s_ref, d):
    """s = +-(1 - min(a, b) / max(a, b)) and the ratio carries <= 2 eps (1 + 4 eps) relative, so
    |s_kernel - s| <= 2 eps (1 - |s|) (1 + 4 eps) (+ 1e-14 for the float64 finish); it holds across a change of the
    arg-min cluster (b is a minimum of perturbed values) and across a = b (s is continuous there)."""
    e = _sil_eps(d)
    return 2.0 * e * (1.0 - np.abs(np.asarray(s_ref, dtype=np.float64))) * (1.0 + 4.0 * e) + 1e-14


def score_bound(s_ref, d):
    return float(np.mean(samples_bound(s_ref, d)))


def silhouette_sums_f32(X, labels):
    """Float32 restatement of the kernel's distance (sequential float32 sum of squared float32 differences, no fma,
    float32 square root) with the float64 cluster sums: what the bounds above must contain."""
    X = np.asarray(X, dtype=np.float32)
    lab, k = _encode(labels)
    n, d = X.shape
    onehot = np.zeros((n, k))
    onehot[np.arange(n), lab] = 1.0
    s2 = np.zeros((n, n), dtype=np.float32)
    for c in range(d):
        e = X[:, c, None] - X[None, :, c]
        s2 = s2 + e * e
    return np.sqrt(s2).astype(np.float64) @ onehot


def silhouette_score(X, labels):
    return float(np.mean(silhouette_samples(X, labels)))


def davies_bouldin_score(X, labels):
    X = np.asarray(X, dtype=np.float64)
    lab, k = _encode(labels)
    cent = np.stack([X[lab == c].mean(0) for c in range(k)])
    intra = np.array([np.linalg.norm(X[lab == c] - cent[c], axis=1).mean() for c in range(k)])
    cd = np.linalg.norm(cent[:, None, :] - cent[None, :, :], axis=2)
    if np.allclose(intra, 0) or np.allclose(cd, 0):
        return 0.0
    cd[cd == 0] = np.inf
    return float(np.mean(np.max((intra[:, None] + intra[None, :]) / cd, axis=1)))


def calinski_harabasz_score(X, labels):
    X = np.asarray(X, dtype=np.float64)
    lab, k = _encode(labels)
    n = X.shape[0]
    mean = X.mean(0)
    extra, intra = 0.0, 0.0
    for c in range(k):
        xc = X[lab == c]
        mc = xc.mean(0)
        extra += len(xc) * ((mc - mean) ** 2).sum()
        intra += ((xc - mc) ** 2).sum()
    return float(1.0 if intra == 0.0 else extra * (n - k) / (intra * (k - 1.0)))


def cluster_stats(X, labels):
    """Centroids, grand mean, mean distance to the own centroid, Davies-Bouldin and Calinski-Harabasz of the float32
    rows X, evaluated in numpy longdouble (64-bit mantissa: its own error is 2^-11 of the bounds below) with the
    sklearn branches, and a bound on |float64 evaluation - this| for each, counted from float64 roundings
    (u = 2^-53) for ANY summation order:

      cent[c][j]  n_c terms summed, one division:                     (n_c + 1) u mean_i |x_ij| + 2u |cent|
      mean[j]     n terms, one division:                              (n + 1) u mean_i |x_ij| + 2u |mean|
                  (the first term is 0 where the float32 column sums are exact in float64 in any order)
      dist_i      ||x_i - cent'|| with cent' off by dc (triangle inequality) + d-term sum of squares + sqrt:
                                                                      ||dc|| + (d / 2 + 3) u dist_i
      intra[c]    n_c distances summed, one division:                 ||dc_c|| + (d / 2 + n_c + 4) u intra_c
      W = sum_i dist_i^2:    sum_i (2 dist_i ||dc|| + ||dc||^2) + (d + n + 3) u W
      B = sum_c n_c ||cent_c - mean||^2, g = cent_c - mean off by e_j = dc_cj + dm_j:
                             sum_c n_c sum_j (2 |g_j| e_j + e_j^2) + (d + k + 4) u B
      CH = B (n - k) / (W (k - 1)):  CH ((1 + rel B) (1 + 4u) / (1 - rel W) - 1)
      cd_ab = ||cent_a - cent_b||:   dcd = ||dc_a|| + ||dc_b|| + (d / 2 + 3) u cd
      R_ab = (intra_a + intra_b) / cd_ab:  (dI_a + dI_b) / (cd - dcd) + R (dcd / (cd - dcd) + 2u); a maximum over b is
             1-Lipschitz, so DB = mean_a max_b R_ab moves by <= mean_a max_b dR_ab + (k + 1) u DB.
    Where two centroids coincide exactly (cd_ab = 0) sklearn's R_ab is 0; the bound keeps 0 there, which holds for
    inputs whose cluster sums are exact in float64 (the degenerate test sets are small integers)."""
    LD = np.longdouble
    u = 2.0 ** -53
    Xf = np.asarray(X, dtype=np.float32)
    X = Xf.astype(LD)
    A = np.abs(Xf.astype(np.float64))
    lab, k = _encode(labels)
    n, d = X.shape
    cnt = np.bincount(lab, minlength=k)
    cent = np.stack([X[lab == c].sum(0) / LD(cnt[c]) for c in range(k)])
    mean = X.sum(0) / LD(n)
    # where every float64 partial sum is exact (scaler_oracle.sums_exact) only the division rounds, and this
    # reference rounds it twice (longdouble, then float64): one float64 spacing, <= 2u |value|, covers both
    cent_b = np.stack([np.where(sums_exact(A[lab == c]), 0.0, (cnt[c] + 1) * u * A[lab == c].mean(0))
                       for c in range(k)]) + 2 * u * np.abs(cent.astype(np.float64))
    mean_b = np.where(sums_exact(A), 0.0, (n + 1) * u * A.mean(0)) + 2 * u * np.abs(mean.astype(np.float64))
    dc = np.sqrt((cent_b ** 2).sum(1))                                      # ||dc_c||
    dist = np.sqrt(((X - cent[lab]) ** 2).sum(1))
    dist64 = dist.astype(np.float64)
    intra = np.array([dist[lab == c].sum() / LD(cnt[c]) for c in range(k)], dtype=LD)
    intra64 = intra.astype(np.float64)
    intra_b = dc + (d / 2.0 + cnt + 4) * u * intra64
    W = (dist ** 2).sum()
    W_b = float((2 * dist64 * dc[lab] + dc[lab] ** 2).sum() + (d + n + 3) * u * float(W))
    g = np.abs((cent - mean[None, :]).astype(np.float64))
    e = cent_b + mean_b[None, :]
    B = (cnt.astype(LD) * ((cent - mean[None, :]) ** 2).sum(1)).sum()
    B_b = float((cnt * (2 * g * e + e * e).sum(1)).sum() + (d + k + 4) * u * float(B))
    if W == 0:
        ch, ch_b = 1.0, 0.0
    else:
        ch = float(B * LD(n - k) / (W * LD(k - 1)))
        rel_b = B_b / float(B) if B > 0 else 0.0
        ch_b = ch * ((1 + rel_b) * (1 + 4 * u) / (1 - W_b / float(W)) - 1) + (B_b if B == 0 else 0.0)
    cd = np.sqrt(((cent[:, None, :] - cent[None, :, :]) ** 2).sum(2)).astype(np.float64)
    if np.allclose(intra64, 0) or np.allclose(cd, 0):
        db, db_b = 0.0, 0.0
    else:
        dcd = dc[:, None] + dc[None, :] + (d / 2.0 + 3) * u * cd
        with np.errstate(divide="ignore", invalid="ignore"):
            R = np.where(cd == 0, 0.0, (intra64[:, None] + intra64[None, :]) / cd)
            dR = np.where(cd == 0, 0.0, (intra_b[:, None] + intra_b[None, :]) / (cd - dcd) + R * (dcd / (cd - dcd) + 2 * u))
        db = float(R.max(1).mean())
        db_b = float(dR.max(1).mean() + (k + 1) * u * db)
    return dict(counts=cnt, cent=cent.astype(np.float64), cent_bound=cent_b, mean=mean.astype(np.float64),
                mean_bound=mean_b, intra=intra64, intra_bound=intra_b, db=db, db_bound=db_b, ch=ch, ch_bound=ch_b)
