"""The model-free and autoencoder rows of the reference's comparison table (src/Conditional_VAE.py:415-452), on the
device: the same K-Means evaluation as ``decomposition.pca_kmeans_baseline`` on other features.

  direct_kmeans_baseline       "Direct Spectral": K-Means on the feature vectors themselves
  autoencoder_kmeans_baseline  "Autoencoder + K-Means": train SimpleAutoencoder on them, cluster its latents
"""
from __future__ import annotations

import torch

from . import _lib as L
from .decomposition import kmeans_scores
from .models import SimpleAutoencoder
from .train import fit_autoencoder


def direct_kmeans_baseline(X, n_clusters, *, y_true=None, random_state=42, n_init=10, device=None):
    """K-Means on X itself.  Returns ``(features, labels, scores)`` as ``pca_kmeans_baseline`` does; features is X as
    the float32 device tensor the kernels read."""
    feats = L.device_matrix(X, device, finite=True)
    labels, scores = kmeans_scores(feats, n_clusters, y_true=y_true, random_state=random_state, n_init=n_init)
    return feats, labels, scores


def autoencoder_kmeans_baseline(X, latent_dim, n_clusters, *, y_true=None, epochs=50, batch_size=32, lr=1e-3, seed=42,
                                random_state=42, n_init=10, compute_dtype="fp32", device=None):
    """``torch.manual_seed(seed)``; ``SimpleAutoencoder(d, latent_dim)``; the reference's training loop
    (``fit_autoencoder``: DataLoader order from the global generator, Adam, mse_loss); ``ae.eval()``; ``_, z = ae(X)``;
    K-Means on z and its scores.  Returns ``(features, labels, scores, loss_history)``: z as a float32 device tensor,
    the int32 labels, the score dict of ``pca_kmeans_baseline`` and the per-epoch mean batch loss (float64 numpy)."""
    Xd = L.device_matrix(X, device, finite=True)
    torch.manual_seed(seed)
    ae = SimpleAutoencoder(Xd.shape[1], latent_dim, compute_dtype=compute_dtype).to(Xd.device)
    history = fit_autoencoder(ae, Xd, epochs=epochs, batch_size=batch_size, lr=lr)
    ae.eval()
    feats = ae.encode(Xd)
    labels, scores = kmeans_scores(feats, n_clusters, y_true=y_true, random_state=random_state, n_init=n_init)
    return feats, labels, scores, history
