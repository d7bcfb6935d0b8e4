"""The model-free and autoencoder rows of the reference's comparison table (src/Conditional_VAE.py:415-452), on the
device: the same K-Means evaluation as ``decomposition.pca_kmeans_baseline`` on other features.

  direct_kmeans_baseline       "Direct Spectral": K-Means on the feature vectors themselves
  autoencoder_kmeans_baseline  "Autoencoder + K-Means": train SimpleAutoencoder on them, cluster its latents
  simple_vae_experiment        the whole first script (src/Simple_VAE.py:131-295): train the Simple VAE, choose k by
                               silhouette, and the "VAE + KMeans" / "PCA + KMeans" rows of its table
  convolutional_vae_experiment the whole second script (src/Convolutional_VAE.py:59-66, 202-459): split, train the Hybrid
                               VAE, latents, the three sweeps and the four 'Convolutional VAE' rows
  conditional_vae_experiment   the whole third script (src/Conditional_VAE.py:368-463): split, train the CVAE, latents and
                               the four 'Conditional VAE' rows
"""
from __future__ import annotations

import numpy as np
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


# ----------------------------------------------------------------------------------------- the convolutional scripts
def conv_vae_algorithm_names(best_k_kmeans, best_k_agg, best_eps):
    """The four 'Algorithm' names of src/Convolutional_VAE.py:378-383, formatted as the script formats them."""
    return [f"K-Means-Main (k={best_k_kmeans})", "K-Means-Language (k=2)", f"Agglomerative (k={best_k_agg})",
            f"DBSCAN (eps={best_eps:.1f})"]


def conv_vae_row(name, labels, scores):
    """One record of src/Convolutional_VAE.py:395-426 from a labelling and its scores (``scores``: a dict with
    'Silhouette', 'Davies-Bouldin' and 'ARI' -- None without ground truth -- or a callable returning one, called only
    when the labelling has more than one cluster; noise, label -1, is no cluster): fewer than 2 clusters give the
    script's -1 row."""
    labels = np.asarray(labels)
    n_clusters = len(set(labels.tolist())) - (1 if -1 in labels else 0)
    if n_clusters > 1:
        sc = scores() if callable(scores) else scores
        vals = (float(sc["Silhouette"]), float(sc["Davies-Bouldin"]), None if sc["ARI"] is None else float(sc["ARI"]))
    else:
        vals = (-1, -1, -1)
    return {"Algorithm": name, "Silhouette": vals[0], "Davies-Bouldin": vals[1], "ARI": vals[2],
            "n_clusters": n_clusters, "Architecture": "Convolutional VAE"}


def cvae_row(method, scores):
    """One record of src/Conditional_VAE.py:410-463 from ``kmeans_scores``' dict: the script's columns in its order."""
    return {**{k: float(scores[k]) for k in ("Silhouette", "NMI", "ARI", "Purity")}, "Method": method,
            "Architecture": "Conditional VAE"}


def convolutional_vae_experiment(audio, text, labels=None, latent_dim=128, seed=42, **fit_kwargs):
    """src/Convolutional_VAE.py:59-66 and 202-459 on the device: ``torch.manual_seed(seed)``; the 85 / 15 split;
    ``HybridVAE(latent_dim, text_dim, input_hw)`` shaped by the data; ``fit_conv_vae`` (``fit_kwargs`` go to it);
    ``extract_latents`` in chunks of the fit's batch size; the three sweeps (``kmeans_k_sweep``,
    ``agglomerative_k_sweep``, ``dbscan_eps_sweep``, whose best-parameter rules are the script's); the four final
    labellings of :378-383 -- taken from the sweeps where a sweep already produced that fit -- and their silhouette,
    Davies-Bouldin and (with ``labels``) ARI.

    Returns a dict: ``latents`` (float32 device tensor), ``fit`` (the ``ConvFitResult``), ``model`` (in eval mode),
    ``best_k_kmeans``, ``best_k_agg``, ``best_eps``, ``kmeans_main_labels``, ``kmeans_language_labels``,
    ``agglomerative_labels``, ``dbscan_labels`` and ``rows``: the four records ``{'Algorithm', 'Silhouette',
    'Davies-Bouldin', 'ARI', 'n_clusters', 'Architecture': 'Convolutional VAE'}`` ready for
    ``results.write_clustering_metrics``."""
    from . import metrics as M
    from .cluster import (DBSCAN, AgglomerativeClustering, KMeans, agglomerative_k_sweep, dbscan_eps_sweep,
                          kmeans_k_sweep)
    from .models import HybridVAE
    from .train import extract_latents, fit_conv_vae, random_split_indices, split_sizes
    n, (H, W) = audio.shape[0], audio.shape[-2:]
    torch.manual_seed(seed)
    if "split" not in fit_kwargs:   # the script splits before it builds the model
        fit_kwargs["split"] = random_split_indices(n, split_sizes(n, fit_kwargs.get("val_fraction", 0.15)),
                                                   fit_kwargs.get("generator"))
    model = HybridVAE(latent_dim, text.shape[1], (int(H), int(W))).cuda()
    fit = fit_conv_vae(model, audio, text, **fit_kwargs)
    latents = extract_latents(model, audio, text, batch_size=fit_kwargs.get("batch_size", 32))
    best_k, km = kmeans_k_sweep(latents)
    best_k_agg, ag = agglomerative_k_sweep(latents)
    best_eps, db = dbscan_eps_sweep(latents)

    def from_sweep(records, key, value, refit):
        rec = next((r for r in records if r[key] == value), None)
        return (refit(), None) if rec is None else (rec["labels"], rec["silhouette"])

    fits = [from_sweep(km, "k", best_k, lambda: KMeans(n_clusters=best_k, random_state=42, n_init=10).fit_predict(latents)),
            from_sweep(km, "k", 2, lambda: KMeans(n_clusters=2, random_state=42, n_init=10).fit_predict(latents)),
            from_sweep(ag, "k", best_k_agg, lambda: AgglomerativeClustering(n_clusters=best_k_agg).fit_predict(latents)),
            from_sweep(db, "eps", best_eps, lambda: DBSCAN(eps=best_eps, min_samples=5).fit_predict(latents))]
    rows = []
    for name, (lab, sil) in zip(conv_vae_algorithm_names(best_k, best_k_agg, best_eps), fits):
        def scores(lab=lab, sil=sil):
            return {"Silhouette": M.silhouette_score(latents, lab) if sil is None else sil,
                    "Davies-Bouldin": M.davies_bouldin_score(latents, lab),
                    "ARI": None if labels is None else M.adjusted_rand_score(labels, lab)}
        rows.append(conv_vae_row(name, lab, scores))
    return {"latents": latents, "fit": fit, "model": model, "best_k_kmeans": best_k, "best_k_agg": best_k_agg,
            "best_eps": best_eps, "kmeans_main_labels": fits[0][0], "kmeans_language_labels": fits[1][0],
            "agglomerative_labels": fits[2][0], "dbscan_labels": fits[3][0], "rows": rows}


def conditional_vae_experiment(audio, text, cond, y_true, handcrafted, latent_dim=64, seed=42, pca_components=None,
                               **fit_kwargs):
    """src/Conditional_VAE.py:368-463 on the device: ``torch.manual_seed(seed)``; the 85 / 15 split;
    ``ConditionalVAE(latent_dim, text_dim, num_classes, input_hw)`` shaped by the data; ``fit_conv_vae``
    (``fit_kwargs`` go to it; the script's CONFIG is ``epochs=600, lr=1e-4``); the latents of the whole set in one
    call; then the four rows, each a K-Means with k = the number of classes in ``y_true`` and its scores: the CVAE's
    latents, ``pca_kmeans_baseline`` / ``autoencoder_kmeans_baseline`` / ``direct_kmeans_baseline`` on ``handcrafted``.
    ``pca_components`` None is the script's ``PCA(n_components=latent_dim)``, which needs at least latent_dim rows and
    handcrafted columns (sklearn raises below that too); a smaller data set names its own count.

    Returns a dict: ``latents``, ``fit`` (the ``ConvFitResult``), ``model`` (in eval mode), ``n_clusters``,
    ``cvae_labels`` / ``pca_labels`` / ``ae_labels`` / ``direct_labels`` and ``rows``: the four records ``{'Silhouette',
    'NMI', 'ARI', 'Purity', 'Method', 'Architecture': 'Conditional VAE'}`` ready for
    ``results.write_clustering_metrics``."""
    from .models import ConditionalVAE
    from .train import extract_latents, fit_conv_vae, random_split_indices, split_sizes
    n, (H, W) = audio.shape[0], audio.shape[-2:]
    y_true = np.asarray(y_true)
    k = len(np.unique(y_true))
    torch.manual_seed(seed)
    if "split" not in fit_kwargs:   # the script splits before it builds the model
        fit_kwargs["split"] = random_split_indices(n, split_sizes(n, fit_kwargs.get("val_fraction", 0.15)),
                                                   fit_kwargs.get("generator"))
    model = ConditionalVAE(latent_dim, text.shape[1], cond.shape[1], (int(H), int(W))).cuda()
    fit = fit_conv_vae(model, audio, text, cond, **fit_kwargs)
    latents = extract_latents(model, audio, text, cond, batch_size=None)
    cvae_labels, cvae_scores = kmeans_scores(latents, k, y_true=y_true)
    _, pca_labels, pca_scores = pca_kmeans_baseline(handcrafted, latent_dim if pca_components is None else pca_components,
                                                    k, y_true=y_true, device=latents.device)
    _, ae_labels, ae_scores, _ = autoencoder_kmeans_baseline(handcrafted, latent_dim, k, y_true=y_true,
                                                             device=latents.device)
    _, direct_labels, direct_scores = direct_kmeans_baseline(handcrafted, k, y_true=y_true, device=latents.device)
    rows = [cvae_row(m, s) for m, s in (("CVAE (Multi-Modal)", cvae_scores), ("PCA + K-Means", pca_scores),
                                        ("Autoencoder + K-Means", ae_scores), ("Direct Spectral", direct_scores))]
    return {"latents": latents, "fit": fit, "model": model, "n_clusters": k, "cvae_labels": cvae_labels,
            "pca_labels": pca_labels, "ae_labels": ae_labels, "direct_labels": direct_labels, "rows": rows}
