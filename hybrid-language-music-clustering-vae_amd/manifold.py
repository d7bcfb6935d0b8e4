"""t-SNE (sklearn.manifold.TSNE) on the GPU, with the repulsive term summed exactly over all pairs.

Replaces ``TSNE(n_components=2, random_state=42[, perplexity=30]).fit_transform(latents)`` at src/Simple_VAE.py:302-303,
src/Convolutional_VAE.py:468-469 and src/Conditional_VAE.py:515-517.

The objective is that of sklearn 1.7's ``method='barnes_hut'``: sparse affinities P over the
``min(n - 1, int(3 perplexity + 1))`` nearest neighbours and a Student-t Q with one degree of freedom.  The repulsive
sum and Z run over all pairs, which is what sklearn computes at ``angle=0``; there is no tree and no approximation
parameter, so ``angle`` is accepted and unused.

Device (libhlmc, include/hlmc.h): the float64 kNN (``hlmc_tsne_knn``), sklearn's perplexity search and the
symmetrised CSR matrix (``hlmc_tsne_affinities``), the gradient and sklearn's gradient-descent iterations
(``hlmc_tsne_run``).  Host: the initial embedding (this package's exact PCA, scaled as sklearn does, or a seeded
normal draw) and sklearn's control loop, which reads back two doubles at each convergence check (every 50
iterations).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

_MAX_SAMPLES = 131072
_MAX_FEATURES = 4096
_MAX_NEIGHBORS = 512
_EXPLORATION_MAX_ITER = 250      # sklearn's TSNE._EXPLORATION_MAX_ITER
_N_ITER_CHECK = 50               # sklearn's TSNE._N_ITER_CHECK


def n_neighbors_for(n_samples, perplexity):
    """sklearn's neighbour count for the Barnes-Hut affinities."""
    return min(n_samples - 1, int(3.0 * perplexity + 1))


class Affinities:
    """The kNN graph and the joint probabilities of ``X`` on its device: ``nbr_idx`` [n][k] int32, ``nbr_d2`` [n][k]
    float64, ``beta`` [n] and ``cond_p`` [n][k] float64, and the CSR matrix ``indptr`` (int64), ``indices`` (int32,
    ascending in each row), ``values`` (float32); ``ws`` is the workspace the gradient calls reuse."""

    def __init__(self, Xd, perplexity):
        n, d = Xd.shape
        k = n_neighbors_for(n, perplexity)
        lib, dev = L.lib(), Xd.device
        self.n, self.d, self.k = n, d, k
        self.ws_bytes = int(lib.hlmc_tsne_workspace(n, d, k))
        if self.ws_bytes <= 0:
            raise ValueError(f"TSNE: n_samples={n}, n_features={d}, n_neighbors={k} are outside the supported range "
                             f"(2..{_MAX_SAMPLES}, 1..{_MAX_FEATURES}, 1..{_MAX_NEIGHBORS})")
        with torch.cuda.device(dev):
            self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
            self.nbr_idx = torch.empty(n, k, dtype=torch.int32, device=dev)
            self.nbr_d2 = torch.empty(n, k, dtype=torch.float64, device=dev)
            self.beta = torch.empty(n, dtype=torch.float64, device=dev)
            self.cond_p = torch.empty(n, k, dtype=torch.float64, device=dev)
            self.indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
            self.indices = torch.empty(2 * n * k, dtype=torch.int32, device=dev)
            self.values = torch.empty(2 * n * k, dtype=torch.float32, device=dev)
            L.check(lib.hlmc_tsne_knn(L.stream(), Xd.data_ptr(), n, d, k, self.nbr_idx.data_ptr(),
                                      self.nbr_d2.data_ptr(), self.ws.data_ptr(), self.ws_bytes), "hlmc_tsne_knn")
            L.check(lib.hlmc_tsne_affinities(L.stream(), self.nbr_idx.data_ptr(), self.nbr_d2.data_ptr(), n, k,
                                             float(perplexity), self.beta.data_ptr(), self.cond_p.data_ptr(),
                                             self.indptr.data_ptr(), self.indices.data_ptr(), self.values.data_ptr(),
                                             self.ws.data_ptr(), self.ws_bytes), "hlmc_tsne_affinities")

    def csr(self):
        """The joint probabilities as host arrays (indptr, indices, values), cut to the stored entries."""
        indptr = self.indptr.cpu().numpy()
        nnz = int(indptr[-1])
        return indptr, self.indices[:nnz].cpu().numpy(), self.values[:nnz].cpu().numpy()


class Descent:
    """The state of sklearn's ``_gradient_descent`` on the device: ``Y``, ``update`` and ``gains`` [n][2] float32 and
    ``stats`` = (Z, KL divergence, gradient norm) of the last iteration run.  sklearn evaluates an iteration's error
    and gradient norm at the embedding BEFORE that iteration's update; ``Y_before`` keeps that embedding."""

    def __init__(self, aff, Y0):
        dev = aff.ws.device
        self.aff = aff
        self.Y = torch.as_tensor(np.ascontiguousarray(Y0, dtype=np.float32), device=dev).contiguous().clone()
        self.update = torch.zeros_like(self.Y)
        self.gains = torch.ones_like(self.Y)
        self.Y_before = self.Y.clone()
        self.stats = torch.zeros(3, dtype=torch.float64, device=dev)

    def run(self, n_iter, exaggeration, momentum, learning_rate):
        """``n_iter`` iterations on the stream, no host synchronisation: all but the last in one call, a device copy of
        ``Y``, then the last (which leaves the statistics)."""
        if n_iter > 1:
            self._run(n_iter - 1, exaggeration, momentum, learning_rate)
        self.Y_before.copy_(self.Y)
        self._run(1, exaggeration, momentum, learning_rate)

    def _run(self, n_iter, exaggeration, momentum, learning_rate):
        a = self.aff
        with torch.cuda.device(self.Y.device):
            L.check(L.lib().hlmc_tsne_run(L.stream(), self.Y.data_ptr(), self.update.data_ptr(), self.gains.data_ptr(),
                                          a.n, a.indptr.data_ptr(), a.indices.data_ptr(), a.values.data_ptr(),
                                          float(exaggeration), float(momentum), float(learning_rate), int(n_iter),
                                          self.stats.data_ptr(), a.ws.data_ptr(), a.ws_bytes), "hlmc_tsne_run")

    def read_stats(self):
        """(KL divergence, gradient norm) of the last iteration: one copy of two doubles, which waits for the stream."""
        s = self.stats.cpu().numpy()
        return float(s[1]), float(s[2])


def gradient_descent(state, it, max_iter, momentum, exaggeration, learning_rate, n_iter_without_progress,
                     min_grad_norm):
    """sklearn's ``_gradient_descent`` from iteration ``it``: the iterations between two convergence checks are one
    ``hlmc_tsne_run`` call.  Returns (error, index of the last iteration run), as sklearn does."""
    best_error = np.finfo(float).max
    best_iter = i = it
    error = best_error
    while i < max_iter:
        stop = min(max_iter, (i // _N_ITER_CHECK + 1) * _N_ITER_CHECK)   # run iterations i .. stop - 1
        state.run(stop - i, exaggeration, momentum, learning_rate)
        i = stop - 1
        error, grad_norm = state.read_stats()
        if (i + 1) % _N_ITER_CHECK == 0:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
        if i + 1 >= max_iter:
            break
        i += 1
    return error, i


class TSNE:
    """sklearn.manifold.TSNE for float32 data in two dimensions, the Barnes-Hut objective with exact repulsion.

    Arguments and defaults are sklearn's.  Not implemented, each a ``ValueError``: ``n_components != 2``, a metric
    other than 'euclidean', and ``method='exact'`` (a dense P is another objective).  ``angle`` is accepted and unused:
    the result is the ``angle -> 0`` limit.  ``init='pca'`` uses this package's exact ``PCA(2)`` (sklearn: the
    randomized solver seeded by ``random_state``) scaled to a standard deviation of 1e-4 in the first column, and so
    needs 2 <= n_features <= 1024; ``init='random'`` draws
    ``1e-4 * RandomState(random_state).standard_normal((n, 2))`` as sklearn does; an [n, 2] array is used as it is.

    Attributes: ``embedding_`` (float32 numpy), ``kl_divergence_`` (of the exact objective, not a tree estimate),
    ``n_iter_``, ``learning_rate_``, ``n_features_in_``.  ``fit_transform`` returns the embedding as a device tensor.

    Supported sizes: 2 <= n_samples <= 131072, n_features <= 4096, int(3 perplexity + 1) <= 512.
    Out of scope: ``process_group=``, three components, other metrics.
    """

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto",
                 max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, metric="euclidean", init="pca",
                 random_state=None, method="barnes_hut", angle=0.5, device=None):
        if n_components != 2:
            raise ValueError(f"n_components={n_components!r} is not implemented: the device kernels embed in 2 dimensions")
        if metric != "euclidean":
            raise ValueError(f"metric={metric!r} is not implemented: only 'euclidean'")
        if method != "barnes_hut":
            raise ValueError(f"method={method!r} is not implemented: 'barnes_hut' names the objective (sparse kNN "
                             f"affinities); its repulsion is summed exactly here.  'exact' uses a dense P, another "
                             f"objective")
        if isinstance(init, str) and init not in ("pca", "random"):
            raise ValueError(f"init={init!r} must be 'pca', 'random' or an array of shape (n_samples, 2)")
        if not (isinstance(learning_rate, str) and learning_rate == "auto") and not float(learning_rate) > 0.0:
            raise ValueError(f"learning_rate={learning_rate!r} must be 'auto' or a positive number")
        if not float(perplexity) > 0.0 or not float(early_exaggeration) >= 1.0:
            raise ValueError("perplexity must be positive and early_exaggeration at least 1")
        if int(max_iter) < _EXPLORATION_MAX_ITER:
            raise ValueError(f"max_iter={max_iter!r} must be at least {_EXPLORATION_MAX_ITER}")   # as sklearn
        self.n_components, self.perplexity, self.early_exaggeration = n_components, perplexity, early_exaggeration
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, n_iter_without_progress
        self.min_grad_norm, self.metric, self.init, self.random_state = min_grad_norm, metric, init, random_state
        self.method, self.angle, self.device = method, angle, device

    def _initial_embedding(self, Xd, n):
        if not isinstance(self.init, str):
            Y0 = self.init.detach().cpu().numpy() if torch.is_tensor(self.init) else np.asarray(self.init)
            if Y0.shape != (n, 2):
                raise ValueError(f"init has shape {Y0.shape}, expected ({n}, 2)")
            if not np.isfinite(Y0).all():
                raise ValueError("init contains NaN or infinity.")
            return Y0.astype(np.float32)
        if self.init == "random":
            rs = self.random_state if isinstance(self.random_state, np.random.RandomState) \
                else np.random.RandomState(self.random_state)
            return 1e-4 * rs.standard_normal(size=(n, 2)).astype(np.float32)
        from .decomposition import PCA
        T = PCA(n_components=2, device=Xd.device).fit_transform(Xd).cpu().numpy()
        return (T / np.std(T[:, 0]) * 1e-4).astype(np.float32)

    def _fit(self, X):
        shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
        if len(shape) != 2:
            raise ValueError("X must be 2-D [n_samples, n_features]")
        n, d = int(shape[0]), int(shape[1])
        if self.perplexity >= n:
            raise ValueError("perplexity must be less than n_samples")
        if n < 2 or n > _MAX_SAMPLES or d < 1 or d > _MAX_FEATURES:
            raise ValueError(f"TSNE: X of shape ({n}, {d}) is outside the supported range (2..{_MAX_SAMPLES} samples, "
                             f"1..{_MAX_FEATURES} features)")
        if n_neighbors_for(n, self.perplexity) > _MAX_NEIGHBORS:
            raise ValueError(f"TSNE: perplexity={self.perplexity} needs {n_neighbors_for(n, self.perplexity)} "
                             f"neighbours, above the supported {_MAX_NEIGHBORS}")
        if not isinstance(self.init, str):
            init_shape = tuple(self.init.shape) if hasattr(self.init, "shape") else np.shape(self.init)
            if init_shape != (n, 2):
                raise ValueError(f"init has shape {init_shape}, expected ({n}, 2)")
        Xd = L.device_matrix(X, self.device, finite=True)
        if self.learning_rate == "auto":
            self.learning_rate_ = float(np.maximum(n / self.early_exaggeration / 4, 50))
        else:
            self.learning_rate_ = float(self.learning_rate)
        self.n_features_in_ = d
        aff = Affinities(Xd, self.perplexity)
        state = Descent(aff, self._initial_embedding(Xd, n))
        self.affinities_ = aff
        # sklearn's _tsne: 250 iterations with the exaggeration at momentum 0.5, the rest at momentum 0.8
        error, it = gradient_descent(state, 0, _EXPLORATION_MAX_ITER, 0.5, self.early_exaggeration,
                                     self.learning_rate_, _EXPLORATION_MAX_ITER, self.min_grad_norm)
        if it < _EXPLORATION_MAX_ITER or self.max_iter - _EXPLORATION_MAX_ITER > 0:
            error, it = gradient_descent(state, it + 1, int(self.max_iter), 0.8, 1.0, self.learning_rate_,
                                         self.n_iter_without_progress, self.min_grad_norm)
        self.n_iter_ = it
        self.kl_divergence_ = error
        self.embedding_ = state.Y.cpu().numpy()
        self._kl_embedding = state.Y_before.cpu().numpy()      # where kl_divergence_ was evaluated, as in sklearn
        return state.Y

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def fit_transform(self, X, y=None):
        return self._fit(X)
