"""hlmc_amd — MI355X-native hot path of Shahriar1638/Hybrid-Language-Music-Clustering-VAE.

Drop-in surface (reference names):
  HybridVAE, loss_function                     (src/Convolutional_VAE.py)
  ConditionalVAE, cvae_loss_function           (src/Conditional_VAE.py)
  VAE, vae_loss                                (src/Simple_VAE.py)
  melspectrogram, power_to_db, mfcc, extract_mel_spectrogram, mean_std_pool, StandardScaler
                                               (librosa / sklearn calls of src/1_preprocessing*.py)
  KMeans, kmeans_k_sweep                       (sklearn KMeans calls of the three model scripts and their k = 2..14
                                                search, all silhouettes in one distance pass)
  DBSCAN, dbscan_eps_sweep                     (sklearn DBSCAN and the eps search of src/Convolutional_VAE.py)
  AgglomerativeClustering, agglomerative_k_sweep   (sklearn's Ward clustering and its k sweep, same script)
  PCA, pca_kmeans_baseline                     (sklearn PCA and the "PCA + KMeans" rows of src/Simple_VAE.py and
                                                src/Conditional_VAE.py)
  TSNE                                         (sklearn t-SNE, the last step of all three scripts, exact repulsion)
  metrics.silhouette_score / davies_bouldin_score / calinski_harabasz_score / adjusted_rand_score /
  normalized_mutual_info_score / calculate_purity   (the sklearn.metrics evaluation calls)
  silhouette_scores                            (metrics.silhouette_scores: silhouette_score of many labellings of one X,
                                                each pairwise distance computed once -- what the three sweeps call)
  Adam                                         (torch.optim.Adam of the train loops)
  Trainer                                      (fused train step + RCCL data parallel)
  SimpleAutoencoder, fit_autoencoder, autoencoder_kmeans_baseline, direct_kmeans_baseline
                                               (the "Autoencoder + K-Means" and "Direct Spectral" rows of
                                                src/Conditional_VAE.py: the training loop resident on the device)
  fit_vae, PlateauStopper, simple_vae_experiment, results.write_clustering_metrics
                                               (the training procedure and table of src/Simple_VAE.py: DataLoader order,
                                                Adam, ReduceLROnPlateau, early stopping and best-weights restore with
                                                one read-back per epoch; the "VAE + KMeans" / "PCA + KMeans" rows and
                                                the shared clustering_metrics.csv)
  fit_conv_vae, extract_latents, random_split_indices, convolutional_vae_experiment, conditional_vae_experiment
                                               (the training runs and tables of src/Convolutional_VAE.py and
                                                src/Conditional_VAE.py: random_split, shuffled training and unshuffled
                                                validation passes resident on the device, early stopping on the
                                                validation loss with one read-back per epoch; the 'Convolutional VAE'
                                                and 'Conditional VAE' rows)
  pipeline.run_pipeline                        (BASELINE config[4]: 30 s clips -> mel -> scaler -> ConvVAE train ->
                                                latents -> KMeans, resident in HBM)
All compute runs in libhlmc.so (hand-written HIP for gfx950); see include/hlmc.h.
"""
from . import _lib
from .cluster import DBSCAN, AgglomerativeClustering, KMeans, agglomerative_k_sweep, dbscan_eps_sweep, kmeans_k_sweep
from .features import (SPECTRAL_FEATURES, StandardScaler, chroma_stft, extract_mel_spectrogram, extract_spectral_features,
                       mean_std_pool, mel_filterbank, melspectrogram, mfcc, power_to_db, rms, spectral_bandwidth,
                       spectral_centroid, spectral_rolloff, spectral_stats, zero_crossing_rate)
from .decomposition import PCA, pca_kmeans_baseline
from . import decomposition
from .manifold import TSNE
from . import manifold
from . import metrics
from .metrics import silhouette_scores
from . import preprocess
from .losses import cvae_loss_function, loss_function, vae_loss
from .models import VAE, ConditionalVAE, HybridVAE, SimpleAutoencoder
from .optim import Adam
from .train import (AutoencoderTrainer, ConvFitResult, GraphedStep, PlateauStopper, Trainer, VAEFitResult,
                    dataloader_order, extract_latents, fit_autoencoder, fit_conv_vae, fit_vae, random_split_indices)
from . import baselines
from .baselines import (autoencoder_kmeans_baseline, conditional_vae_experiment, convolutional_vae_experiment,
                        direct_kmeans_baseline, simple_vae_experiment)
from . import results
from .results import write_clustering_metrics
from . import pipeline

__all__ = ["HybridVAE", "ConditionalVAE", "VAE", "loss_function", "cvae_loss_function", "vae_loss", "melspectrogram",
           "power_to_db", "mfcc", "extract_mel_spectrogram", "mean_std_pool", "mel_filterbank", "StandardScaler",
           "KMeans", "kmeans_k_sweep", "silhouette_scores", "DBSCAN", "dbscan_eps_sweep", "AgglomerativeClustering",
           "agglomerative_k_sweep",
           "PCA", "pca_kmeans_baseline", "TSNE",
           "Adam", "Trainer", "GraphedStep", "metrics", "SimpleAutoencoder", "AutoencoderTrainer", "dataloader_order",
           "fit_autoencoder", "autoencoder_kmeans_baseline", "direct_kmeans_baseline", "PlateauStopper", "VAEFitResult",
           "fit_vae", "simple_vae_experiment", "write_clustering_metrics", "random_split_indices", "ConvFitResult",
           "fit_conv_vae", "extract_latents", "convolutional_vae_experiment", "conditional_vae_experiment"]
