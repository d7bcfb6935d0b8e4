"""The model-free and autoencoder rows of the reference's comparison table (src/Conditional_VAE.py:415-452), on the
device: the same K-Means evaluation as ``decomposition.pca_kmeans_baseline`` on other features.

  direct_kmeans_baseline       "Direct Spectral": K-Means on the feature vectors themselves
  autoencoder_kmeans_baseline  "Autoencoder + K-Means": train SimpleAutoencoder on them, cluster its latents
  simple_vae_experiment        the whole first script (src/Simple_VAE.py:131-295): train the Simple VAE, choose k by
                               silhouette, and the "VAE + KMeans" / "PCA + KMeans" rows of its table
"""
from __future__ import annotations

import torch

from . import _lib as L
from .decomposition import kmeans_scores, pca_kmeans_baseline
from .models import VAE, SimpleAutoencoder
from .train import fit_autoencoder, fit_vae


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


def simple_vae_experiment(features, hidden_dims=(128, 64, 32), latent_dim=32, k_range=range(3, 10, 2), seed=42,
                          compute_dtype="fp32", device=None, **fit_kwargs):
    """src/Simple_VAE.py:131-295 on the device: ``torch.manual_seed(seed)``; ``VAE(d, hidden_dims, latent_dim)``;
    ``fit_vae`` (``fit_kwargs`` go to it: epochs, batch_size, lr, beta, patience, ...); ``eval()``;
    ``get_latent_features(features)`` in one call; ``kmeans_k_sweep(latents, k_range)``, whose best_k rule is the
    script's; silhouette and Calinski-Harabasz of that labelling; ``pca_kmeans_baseline(features, latent_dim, best_k)``.

    Returns a dict: ``latents`` (float32 device tensor), ``vae_labels`` / ``pca_labels`` (int32), ``best_k``, ``fit``
    (the ``VAEFitResult``), ``model`` (in eval mode, holding the best weights) and ``rows``: the two records
    ``{'Method', 'Silhouette', 'Calinski-Harabasz', 'Architecture': 'Simple VAE'}`` of the script's table, ready for
    ``results.write_clustering_metrics``."""
    from . import metrics as M
    from .cluster import kmeans_k_sweep
    Xd = L.device_matrix(features, device, finite=True)
    torch.manual_seed(seed)
    vae = VAE(Xd.shape[1], list(hidden_dims), latent_dim, compute_dtype=compute_dtype).to(Xd.device)
    fit = fit_vae(vae, Xd, **fit_kwargs)
    vae.eval()
    latents = vae.get_latent_features(Xd)
    best_k, records = kmeans_k_sweep(latents, k_range, random_state=42, n_init=10, device=Xd.device)
    rec = next((r for r in records if r["k"] == best_k), None)
    if rec is None:  # no k of the range beat the script's starting point (2, -1)
        vae_labels, vae_scores = kmeans_scores(latents, best_k)
    else:
        vae_labels = rec["labels"]
        vae_scores = {"Silhouette": rec["silhouette"],
                      "Calinski-Harabasz": M.calinski_harabasz_score(latents, vae_labels)}
    _, pca_labels, pca_scores = pca_kmeans_baseline(Xd, latent_dim, best_k, device=Xd.device)
    rows = [{"Method": method, "Silhouette": float(sc["Silhouette"]),
             "Calinski-Harabasz": float(sc["Calinski-Harabasz"]), "Architecture": "Simple VAE"}
            for method, sc in (("VAE + KMeans", vae_scores), ("PCA + KMeans", pca_scores))]
    return {"latents": latents, "vae_labels": vae_labels, "pca_labels": pca_labels, "best_k": best_k, "fit": fit,
            "model": vae, "rows": rows}
