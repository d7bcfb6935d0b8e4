// Internal declarations of the feature (mel / MFCC / scaler) and K-Means kernels.
#pragma once
#include <vector>

#include "ops.hpp"

namespace hlmc {

struct MelPlanImpl {
    int sr, n_fft, hop, n_mels;
    double fmin, fmax;
    int nbins;                       // 1 + n_fft/2
    std::vector<float> dense;        // [n_mels][nbins] (host copy, librosa.filters.mel)
    // device tables
    float* d_window = nullptr;       // [n_fft]
    float2* d_tw = nullptr;          // FFT twiddles: W1024^{p k1} [15][64], radix-2 lane stages [5][64]
    float2* d_rtw = nullptr;         // [n_fft/2+1] e^{-2 pi i f / n_fft}
    int* d_band = nullptr;           // [n_mels][2] first bin, count
    int* d_woff = nullptr;           // [n_mels] offset into d_w
    float* d_w = nullptr;            // packed weights
    int max_band = 0;
    int nnz = 0;
    // chroma_stft tables (built on first use): 99 filterbanks [12][1028] f32 (one per tuning edge), edges
    float* d_chroma_fb = nullptr;
    double* d_tune_edges = nullptr;
    int pip_kmin = -1, pip_kmax = 0;
};

namespace feat {
int plan_create(int sr, int n_fft, int hop, int n_mels, double fmin, double fmax, MelPlanImpl** out);
void plan_destroy(MelPlanImpl* p);
int test_stft_grid(int blocks);  // test hook: 0 = default grid, else that many blocks (a multiple of 8)
int64_t frames(const MelPlanImpl* p, int64_t n);
int64_t workspace(const MelPlanImpl* p, int64_t B, int64_t n);
int melspectrogram(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, float* out, void* ws);
int mel_db(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, int64_t t_keep, float amin,
           float top_db, float* out, void* ws);
int mel_db_zscore(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, int64_t t_keep,
                  float amin, float top_db, const double* mean, const double* scale, int dtype, void* out, void* ws);
int mfcc(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, int n_mfcc, const float* dct,
         float amin, float top_db, float* out, void* ws);
int power_to_db(hipStream_t s, const float* S, int64_t B, int64_t per, int ref_max, float ref_value, float amin,
                float top_db, float* out, void* ws);
int spectral_shape(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, double roll_percent,
                   double* out);
int zcr_rms(const MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, double* zcr, float* rms);
int64_t chroma_workspace(const MelPlanImpl* p, int64_t B, int64_t n);
int chroma_stft(MelPlanImpl* p, hipStream_t s, const float* pcm, int64_t B, int64_t n, float* out, double* tuning,
                void* ws);
int row_mean_std(hipStream_t s, const float* x, int64_t rows, int64_t cols, float* mean, float* sd);
int64_t colstats_workspace(int64_t n, int64_t cols);
int colstats(hipStream_t s, const float* x, int64_t n, int64_t cols, const double* mean, double* o0, double* o1, void* ws);
int zscore(hipStream_t s, const float* x, int64_t n, int64_t cols, const double* mean, const double* scale, int dtype,
           void* out);
}  // namespace feat

namespace km {
int center(hipStream_t s, const float* X, int64_t n, int d, float* mean, float* var, float* Xc);
int sqdist_rows(hipStream_t s, const float* X, int64_t n, int d, const int64_t* cand, int ncand, float* out);
int assign(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, int32_t* labels, const int32_t* old,
           int32_t* n_changed);
int sums(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sm, float* w);
size_t sums_ws(int64_t n, int k);
int sums_part(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sm, float* w,
              void* ws, size_t ws_bytes);
int inertia(hipStream_t s, const float* X, int64_t n, int d, const float* C, const int32_t* labels, float* out,
            float* tmp);
int rowdist(hipStream_t s, const float* X, int64_t n, int d, const float* C, const int32_t* labels, float* out);
// restart-batched (R restarts in lockstep; active = bitmask of the restarts to run)
int assign_batch(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, int R, uint64_t active,
                 int32_t* labels, const int32_t* old, int32_t* n_changed);
int sums_batch(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, int R, uint64_t active,
               float* sm, float* w, void* ws, size_t ws_bytes);
int update_batch(hipStream_t s, int k, int d, int R, uint64_t active, const float* sm, const float* w,
                 const float* C_old, float* C_new, float* info);
int pp_search(hipStream_t s, int64_t n, int R, int T, const float* prev, int prevT, const int32_t* best,
              const double* rvals, int64_t* cand, int32_t* amb);
int pp_dist(hipStream_t s, const float* X, int64_t n, int d, int R, int T, const int64_t* cand, const float* prev,
            int prevT, const int32_t* best, float* out);
int inertia_batch(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, const int32_t* labels, int R,
                  float* out, float* tmp);
}  // namespace km

// cluster-quality metrics (metrics.hip): silhouette (sklearn silhouette_score / silhouette_samples),
// Davies-Bouldin + Calinski-Harabasz.  Labels are 0..k-1 int32.
namespace metrics {
size_t silhouette_workspace(int64_t n, int k);
int silhouette(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, double* samples,
               double* score, void* ws, size_t ws_bytes);
// M labellings of one X in one distance pass (labels [M][n], row m in [0, ks[m]); ks is a host array); each
// labelling's S columns, counts, samples and score have the bits silhouette() gives for it alone
size_t silhouette_batch_workspace(int64_t n, const int32_t* ks, int M);   // 0: arguments out of range
int silhouette_batch(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, const int32_t* ks, int M,
                     double* samples, double* scores, void* ws, size_t ws_bytes);
size_t cluster_scores_workspace(int k, int d);
int cluster_scores(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, double* out2,
                   void* ws, size_t ws_bytes);
}  // namespace metrics

// DBSCAN with sklearn's labels (dbscan.hip): one neighbourhood pass for up to 32 squared radii (bit-packed
// adjacency in the workspace, per-row neighbour counts, borderline-pair counts), then a labelling pass per radius.
namespace dbscan {
size_t workspace(int64_t n, int E);
int neighbors(hipStream_t s, const float* X, int64_t n, int d, const double* radii_sq, int E, int32_t* counts,
              uint64_t* borderline, void* ws, size_t ws_bytes);
int labels(hipStream_t s, int64_t n, int E, int e, int min_samples, const int32_t* counts, void* ws, size_t ws_bytes,
           int32_t* labels_out, uint8_t* core_out, int32_t* n_clusters);
}  // namespace dbscan

// Ward agglomerative clustering with sklearn's tree (ward.hip): the full float64 distance matrix in scipy's pdist
// arithmetic, then the nearest-neighbour chain with the Lance-Williams update in one launch of one workgroup.
namespace ward {
size_t workspace(int64_t n);
int pdist(hipStream_t s, const float* X, int64_t n, int d, double* D);
int chain(hipStream_t s, int64_t n, double* D, int32_t* merge_a, int32_t* merge_b, double* merge_dist,
          int32_t* merge_size, void* ws, size_t ws_bytes);
}  // namespace ward

// PCA (pca.hip): the float64 column mean and centred Gram matrix of float32 rows, and the float64-accumulated
// projection out = (A - a_off) B + o_off, both on the fp64 MFMA; the d x d eigen-solve stays on the host.
namespace pca {
size_t workspace(int64_t n, int d);
int cov(hipStream_t s, const float* X, int64_t n, int d, double* mean, double* G, void* ws, size_t ws_bytes);
int project(hipStream_t s, const float* A, int64_t n, int p, const double* B, int q, const double* a_off,
            const double* o_off, float* out);
}  // namespace pca

// t-SNE (tsne.hip): kNN on the fp64 MFMA, sklearn's perplexity search and the symmetrised CSR affinities, the exact
// all-pairs gradient of the Barnes-Hut objective, and sklearn's gradient-descent iterations, all on the stream.
namespace tsne {
size_t workspace(int64_t n, int d, int k);
int knn(hipStream_t s, const float* X, int64_t n, int d, int k, int32_t* nbr_idx, double* nbr_d2, void* ws,
        size_t ws_bytes);
int affinities(hipStream_t s, const int32_t* nbr_idx, const double* nbr_d2, int64_t n, int k, double perplexity,
               double* beta, double* cond_p, int64_t* indptr, int32_t* indices, float* values, void* ws,
               size_t ws_bytes);
int gradient(hipStream_t s, const float* Y, int64_t n, const int64_t* indptr, const int32_t* indices,
             const float* values, double exaggeration, float* grad, double* stats, int want_stats, void* ws,
             size_t ws_bytes);
int run(hipStream_t s, float* Y, float* update, float* gains, int64_t n, const int64_t* indptr,
        const int32_t* indices, const float* values, double exaggeration, double momentum, double learning_rate,
        int n_iter, double* stats, void* ws, size_t ws_bytes);
}  // namespace tsne

// The SimpleAutoencoder train step's feed and loss (autoencoder.hip): the step's rows gathered into a static padded
// batch with the row count left in device memory, and the mean squared error over that many rows with its gradient.
namespace ae {
int batch_gather(hipStream_t s, const float* X, int64_t n, int d, const int64_t* idx, int count, int B, float* out,
                 int* valid_dev);
size_t mse_rows_workspace(int64_t B, int64_t d);   // 0: arguments out of range
int mse_rows(hipStream_t s, const float* recon, const float* target, int B, int d, const int* valid_dev, float* d_recon,
             double* sums2, double* acc, void* ws);
// The Simple VAE's epoch means (src/Simple_VAE.py:190-196) from the per-step loss sums left on the device: one thread
// adds the nb steps' recon / kl / total in step order in float64 and divides by nb; out3 = {loss, recon, kl}.
int vae_epoch_means(hipStream_t s, const double* sums, const int64_t* na_nl, int nb, double beta, double* out3);
// The convolutional VAEs' epoch totals (src/Convolutional_VAE.py:237-256, src/Conditional_VAE.py:331-345) from the loss
// sums of the epoch's nt training steps and nv validation batches: one thread, float64, step order;
// out5 = {train total, audio, text, kld} / train_div and {validation total} / val_div.
int fit_epoch_totals(hipStream_t s, const double* train_sums, int nt, const double* val_sums, int nv,
                     double text_weight, double beta, double train_div, double val_div, double* out5);
}  // namespace ae

}  // namespace hlmc
