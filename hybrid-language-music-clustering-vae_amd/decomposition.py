"""PCA (sklearn.decomposition.PCA) with the centred Gram matrix and the projections on the GPU.

Replaces ``PCA(n_components=32).fit_transform(features)`` at src/Simple_VAE.py:258-263 (the "PCA + KMeans" row on the
370-d handcrafted vectors) and ``PCA(n_components=64).fit_transform(data['handcrafted'])`` at
src/Conditional_VAE.py:422-425 (the "PCA + K-Means" row on the 290-d vectors); ``pca_kmeans_baseline`` runs either row
end to end on the device.

Device (libhlmc, float64 on the fp64 MFMA): the column mean and the centred Gram matrix (X - m)^T (X - m) of the
float32 rows (``hlmc_pca_cov``), and every projection (``hlmc_pca_project``: transform, inverse_transform, whitening).
Host: ``numpy.linalg.eigh`` of the d x d Gram matrix, the descending order, the sign rule and the attributes -- the
small sequential step, as Ward's sort and cut are.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _lib as L

_MAX_FEATURES = 1024
_MAX_SAMPLES = 1 << 24


def _project(A, B, a_off, o_off):
    """out [n][q] f32 = (A - a_off) B + o_off on the device; B [p][q], a_off [p], o_off [q]: host float64 or None."""
    n, p = A.shape
    dev = A.device
    Bd = torch.as_tensor(np.ascontiguousarray(B, dtype=np.float64), device=dev)
    q = Bd.shape[1]
    ad = None if a_off is None else torch.as_tensor(np.ascontiguousarray(a_off, dtype=np.float64), device=dev)
    od = None if o_off is None else torch.as_tensor(np.ascontiguousarray(o_off, dtype=np.float64), device=dev)
    out = torch.empty(n, q, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().hlmc_pca_project(L.stream(), A.data_ptr(), n, p, Bd.data_ptr(), q, L.ptr(ad), L.ptr(od),
                                         out.data_ptr()), "hlmc_pca_project")
    return out


def _eig_descending(G):
    """Eigenpairs of the symmetric G, eigenvalues descending (equal ones in eigh's order) and clipped at 0, every
    eigenvector's entry of largest magnitude (first occurrence) positive: sklearn's svd_flip(u_based_decision=False).
    Returns (eigenvalues [d], components [d][d] with the eigenvectors as rows)."""
    lam, vec = np.linalg.eigh(G)
    order = np.argsort(-lam, kind="stable")
    lam = np.maximum(lam[order], 0.0)
    V = np.ascontiguousarray(vec[:, order].T)
    big = np.argmax(np.abs(V), axis=1)
    sign = np.sign(V[np.arange(V.shape[0]), big])
    sign[sign == 0] = 1.0
    return lam, V * sign[:, None]


class PCA:
    """sklearn.decomposition.PCA for float32 data, exact: the eigen-decomposition of the float64 centred Gram matrix.

    ``svd_solver`` 'auto', 'full' and 'covariance_eigh' all run this one exact path; 'randomized' and 'arpack' raise.
    At the reference's shapes (1336 x 370 -> 32, 1336 x 290 -> 64) sklearn's 'auto' would pick the *randomized*
    solver, seeded from ``random_state`` or the global RNG; this class returns the exact decomposition instead, so
    ``random_state`` is accepted and unused.  The contract is a derived rounding bound against the exact PCA
    (tests/pca_check.py), which puts the result closer to it than any of sklearn's float32 solvers (about 1e-6 for
    'full' / 'randomized', 1e-2 for 'covariance_eigh' on data far from the origin).

    ``n_components``: an int in [1, min(n_samples, n_features)], None (= min(n_samples, n_features)) or a float in
    (0, 1) with sklearn's rule (the smallest count whose cumulated variance ratio exceeds it).  'mle' raises.

    Attributes follow sklearn's definitions and dtype (float32): ``components_``, ``explained_variance_``
    (eigenvalue / (n - 1)), ``explained_variance_ratio_`` (over all min(n, d) variances), ``singular_values_``,
    ``mean_``, ``noise_variance_``, ``n_components_``, ``n_samples_``, ``n_features_in_``.  The float64 mean and
    components are kept privately and used by ``transform`` / ``inverse_transform``, which return device tensors.

    Out of scope: ``process_group=`` (a row-sharded Gram matrix), float64 input (it is converted to float32, as the
    other estimators do), more than 1024 features (the reference itself declines PCA on raw mel).
    """

    def __init__(self, n_components=None, *, whiten=False, svd_solver="auto", random_state=None, device=None):
        if svd_solver not in ("auto", "full", "covariance_eigh"):
            raise ValueError(f"svd_solver={svd_solver!r} is not implemented: 'auto', 'full' and 'covariance_eigh' run "
                             f"the exact decomposition, 'randomized' and 'arpack' have no counterpart here")
        if isinstance(n_components, str):
            raise ValueError(f"n_components={n_components!r} is not implemented (an int, None or a float in (0, 1))")
        self.n_components, self.whiten, self.svd_solver = n_components, whiten, svd_solver
        self.random_state, self.device = random_state, device

    def _resolve_components(self, n, d):
        k, m = self.n_components, min(n, d)
        if k is None:
            return m
        if isinstance(k, numbers.Integral) and not isinstance(k, bool):
            if not 1 <= k <= m:
                raise ValueError(f"n_components={k} must be between 1 and min(n_samples, n_features)={m}")
            return int(k)
        if isinstance(k, numbers.Real) and 0.0 < k < 1.0:
            return float(k)
        raise ValueError(f"n_components={k!r} must be an int in [1, {m}], None or a float in (0, 1)")

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def _fit(self, X):
        shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
        if len(shape) != 2:
            raise ValueError("X must be 2-D [n_samples, n_features]")
        n, d = int(shape[0]), int(shape[1])
        if n < 2 or n > _MAX_SAMPLES:
            raise ValueError(f"PCA: n_samples={n} is outside the supported range [2, {_MAX_SAMPLES}]")
        if d > _MAX_FEATURES:
            raise ValueError(f"PCA: n_features={d} is above the supported {_MAX_FEATURES}")
        k = self._resolve_components(n, d)
        Xd = L.device_matrix(X, self.device, finite=True)
        lib = L.lib()
        dev = Xd.device
        ws_bytes = int(lib.hlmc_pca_workspace(n, d))
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            mg = torch.empty(d + d * d, dtype=torch.float64, device=dev)   # mean | G: one copy back
            L.check(lib.hlmc_pca_cov(L.stream(), Xd.data_ptr(), n, d, mg.data_ptr(), mg[d:].data_ptr(), ws.data_ptr(),
                                     ws_bytes), "hlmc_pca_cov")
            mg_h = mg.cpu().numpy()
        mean, G = mg_h[:d], mg_h[d:].reshape(d, d)
        lam, V = _eig_descending(G)
        m = min(n, d)
        lam, V = lam[:m], V[:m]                      # a rank above n - 1 is rounding
        var = lam / (n - 1)
        total = var.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = var / total                      # all-constant X: 0 / 0 = nan, as sklearn
        if isinstance(k, float):
            k = int(np.searchsorted(np.cumsum(ratio), k, side="right")) + 1
            k = min(k, m)
        f32 = np.float32
        self.noise_variance_ = f32(var[k:].mean()) if k < m else 0.0
        self.n_samples_, self.n_components_, self.n_features_in_ = n, k, d
        self._mean64, self._components64, self._variance64 = mean.copy(), V[:k].copy(), var[:k].copy()
        self.mean_ = mean.astype(f32)
        self.components_ = V[:k].astype(f32)
        self.explained_variance_ = var[:k].astype(f32)
        self.explained_variance_ratio_ = ratio[:k].astype(f32)
        self.singular_values_ = np.sqrt(lam[:k]).astype(f32)
        return Xd

    def _scale(self):
        """sklearn's whitening divisor: sqrt(explained_variance_) clipped below at the float32 epsilon."""
        return np.maximum(np.sqrt(self._variance64), float(np.finfo(np.float32).eps))

    def _forward(self, Xd):
        B = self._components64.T
        if self.whiten:
            B = B / self._scale()[None, :]
        return _project(Xd, B, self._mean64, None)

    def fit_transform(self, X, y=None):
        """``fit`` followed by the projection of the same rows (sklearn's U S, or U sqrt(n - 1) when whitening)."""
        return self._forward(self._fit(X))

    def transform(self, X):
        Xd = L.device_matrix(X, self.device, finite=True)
        if Xd.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {Xd.shape[1]} features, but PCA is expecting {self.n_features_in_} features as "
                             f"input.")
        return self._forward(Xd)

    def inverse_transform(self, X):
        Zd = L.device_matrix(X, self.device, finite=True)
        if Zd.shape[1] != self.n_components_:
            raise ValueError(f"X has {Zd.shape[1]} components, but PCA was fitted with {self.n_components_}")
        B = self._components64
        if self.whiten:
            B = np.sqrt(self._variance64)[:, None] * B
        return _project(Zd, B, None, self._mean64)


def kmeans_scores(feats, n_clusters, *, y_true=None, random_state=42, n_init=10):
    """K-Means on the device features and the reference's scores of its labels: ``(labels, scores)``, scores keyed as
    the reference's CSV columns ('Silhouette', 'Calinski-Harabasz'; with ``y_true`` also 'NMI', 'ARI', 'Purity').  The
    evaluation every baseline row shares (``evaluate_clustering`` at src/Conditional_VAE.py:296-308)."""
    from . import metrics as M
    from .cluster import KMeans
    kmeans = KMeans(n_clusters=n_clusters, random_state=random_state, n_init=n_init, device=feats.device)
    labels = kmeans.fit_predict(feats)
    scores = {"Silhouette": M.silhouette_score(feats, labels),
              "Calinski-Harabasz": M.calinski_harabasz_score(feats, labels)}
    if y_true is not None:
        scores["NMI"] = M.normalized_mutual_info_score(y_true, labels)
        scores["ARI"] = M.adjusted_rand_score(y_true, labels)
        scores["Purity"] = M.calculate_purity(y_true, labels)
    return labels, scores


def pca_kmeans_baseline(X, n_components, n_clusters, *, y_true=None, random_state=42, n_init=10, device=None):
    """The reference's baseline row on the device: PCA -> KMeans -> silhouette and Calinski-Harabasz
    (src/Simple_VAE.py:258-263), plus NMI, ARI and purity when ``y_true`` is given (``evaluate_clustering`` at
    src/Conditional_VAE.py:296-308, 422-425).  The PCA features stay on the device between the three stages.

    Returns ``(features, labels, scores)``: the float32 feature tensor on the device, the int32 K-Means labels and a
    dict keyed as the reference's CSV columns ('Silhouette', 'Calinski-Harabasz'; with ``y_true`` also 'NMI', 'ARI',
    'Purity')."""
    feats = PCA(n_components=n_components, device=device).fit_transform(X)
    labels, scores = kmeans_scores(feats, n_clusters, y_true=y_true, random_state=random_state, n_init=n_init)
    return feats, labels, scores
