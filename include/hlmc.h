/* libhlmc — MI355X (gfx950) hot path of Shahriar1638/Hybrid-Language-Music-Clustering-VAE.
 *
 * C ABI: plain device pointers (caller-owned, contiguous, 16-byte aligned), sizes, scalars.
 * Every call is stream-ordered and asynchronous on `stream` (a hipStream_t; NULL = default stream),
 * performs no device allocation and no host<->device synchronisation unless stated.
 * Return 0 (HLMC_OK) on success or a negative hlmc_status; hlmc_last_error() gives a thread-local
 * message.  The library never aborts the process.
 *
 * The reference is pure Python; it has no FFI.  Each entry point below names the reference call it
 * replaces (file:line in the reference repo) — the Python package in
 * hybrid-language-music-clustering-vae_amd/ binds them with ctypes.
 */
#ifndef HLMC_H_
#define HLMC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum hlmc_status {
    HLMC_OK = 0,
    HLMC_EINVAL = -1, /* bad shape / pointer / argument */
    HLMC_EHIP = -2,   /* HIP runtime error */
    HLMC_EUNSUP = -3, /* configuration not supported */
    HLMC_EDEVICE = -4, /* a kernel reported a fault through the device status word (hlmc_device_status) */
};

enum hlmc_dtype { HLMC_F32 = 0, HLMC_BF16 = 1 };

int hlmc_version(void);
const char* hlmc_last_error(void);
/* Device status word: bits a kernel raised instead of hanging or returning silently wrong values (bit 0: the one-launch
 * BatchNorm backward's grid-wide arrival count timed out, its outputs are NaN; bit 1: hlmc_batch_gather met a row index
 * outside [0, n), that row is zeros).  No synchronisation: kernels write it
 * with system-scope stores into pinned host memory, so a launch's bit is visible once the launch has completed.  While a
 * bit is raised, hlmc_net_backward / hlmc_op_bn_bwd return HLMC_EDEVICE.  clear != 0 resets the word.  Returns the bits. */
int hlmc_device_status(int clear);
/* test hook: largest R * C taking the one-launch BatchNorm backward (-1: the default 2^22; 0: two passes everywhere)
 * and the arrival spin's poll bound (-1: the default).  Not for production use. */
int hlmc_test_bn_fused(int64_t max_elems, int spin_max);
/* test hook: the persistent grid of the STFT kernels (mel, spectral shape, piptrack).  0 restores the default (resident
 * blocks, at most one per item); a positive multiple of 8 launches exactly that many blocks, so that a small batch
 * walks several items per block.  Any such grid computes the same values.  Anything else returns HLMC_EINVAL.  Not for
 * production use. */
int hlmc_test_stft_grid(int blocks);

/* ============================================================== features
 * Replaces librosa.feature.melspectrogram + librosa.power_to_db at
 *   src/1_preprocessing_advanced.py:97-114 and src/1_preprocessing.py:48-58,
 * librosa.feature.mfcc at src/1_preprocessing.py:61-70, the mean/std pooling at
 * src/1_preprocessing.py:115-121 and sklearn StandardScaler at src/1_preprocessing_advanced.py:376-382.
 * STFT: center=True (zero pad n_fft/2), periodic Hann, hop; power |X|^2; Slaney mel (norm='slaney'). */
typedef struct hlmc_mel_plan hlmc_mel_plan;

int hlmc_mel_plan_create(int sr, int n_fft, int hop, int n_mels, double fmin, double fmax, hlmc_mel_plan** out);
int hlmc_mel_plan_destroy(hlmc_mel_plan* plan);
/* host copy of the dense [n_mels][1 + n_fft/2] float32 filterbank (librosa.filters.mel) */
int hlmc_mel_filterbank(const hlmc_mel_plan* plan, float* out_host);
int64_t hlmc_mel_frames(const hlmc_mel_plan* plan, int64_t n_samples);
/* bytes of scratch for hlmc_mel_db / hlmc_mfcc */
int64_t hlmc_mel_workspace(const hlmc_mel_plan* plan, int64_t batch, int64_t n_samples);
/* power mel spectrogram: pcm [batch][n_samples] f32 -> out [batch][n_mels][T] f32 (ws: >= 8*batch bytes) */
int hlmc_melspectrogram(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch,
                        int64_t n_samples, float* out, void* ws);
/* extract_mel_spectrogram: mel -> power_to_db(ref=max over ALL frames of the clip, amin, top_db)
 * -> keep the first t_keep frames (pad with the clip minimum if t_keep > T). out [batch][n_mels][t_keep] */
int hlmc_mel_db(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
                int64_t t_keep, float amin, float top_db, float* out, void* ws);
/* hlmc_mel_db followed by StandardScaler.transform (hlmc_zscore_apply with cols = n_mels * t_keep) in the same
 * dB pass: the fitted mel scaler applied to freshly extracted clips (src/1_preprocessing_advanced.py:97-114, then
 * the transform half of mel_scaler.fit_transform at :376-379 on the flattened mel).  Bit-identical to that pair.
 * t_keep % 4 == 0; out [batch][n_mels][t_keep] f32 (16-byte aligned) or bf16 (8-byte aligned). */
int hlmc_mel_db_zscore(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
                       int64_t t_keep, float amin, float top_db, const double* mean, const double* scale,
                       int out_dtype, void* out, void* ws);
/* librosa.power_to_db on a [batch][per_clip] array: ref_max!=0 -> ref = per-clip max, else ref_value
 * (ws: >= 8*batch bytes) */
int hlmc_power_to_db(void* stream, const float* S, int64_t batch, int64_t per_clip, int ref_max, float ref_value,
                     float amin, float top_db, float* out, void* ws);
/* librosa.feature.mfcc(n_mfcc): power_to_db(ref=1.0, top_db=80) then DCT-II ortho over mels.
 * out [batch][n_mfcc][T] */
int hlmc_mfcc(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
              int n_mfcc, float* out, void* ws);
/* Handcrafted spectral features of src/1_preprocessing.py:73-91 and src/1_preprocessing_advanced.py:133-137,
 * same framing as the plan (center=True, periodic Hann, n_fft, hop; T = hlmc_mel_frames):
 * librosa.feature.spectral_centroid / spectral_bandwidth (p=2, norm=True) / spectral_rolloff(roll_percent)
 * on |STFT| (power 1).  out [batch][3][T] f64, rows centroid, bandwidth, rolloff (Hz). */
int hlmc_spectral_shape(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
                        double roll_percent, double* out);
/* librosa.feature.zero_crossing_rate(frame_length=n_fft, hop) (edge padding, threshold 1e-10) -> zcr [batch][T]
 * f64 and librosa.feature.rms(frame_length=n_fft, hop) (zero padding) -> rms [batch][T] f32.  n_fft = 2048. */
int hlmc_zcr_rms(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
                 double* zcr, float* rms);
/* librosa.feature.chroma_stft(y, sr, n_fft, hop) of src/1_preprocessing.py:94-102 and
 * src/1_preprocessing_advanced.py:139-141: power |STFT|^2 -> estimate_tuning (piptrack fmin 150, fmax 4000,
 * threshold 0.1; median-magnitude peaks; 0.01-semitone histogram) -> filters.chroma(tuning) -> norm=inf.
 * out [batch][12][T] f32; tuning [batch] f64 (nullable); ws: hlmc_chroma_workspace bytes. */
int64_t hlmc_chroma_workspace(const hlmc_mel_plan* plan, int64_t batch, int64_t n_samples);
int hlmc_chroma_stft(const hlmc_mel_plan* plan, void* stream, const float* pcm, int64_t batch, int64_t n_samples,
                     float* out, double* tuning, void* ws);
/* mean and std (ddof=0) of each row of x [rows][cols] (the mean/std pooling of the feature vectors) */
int hlmc_row_mean_std(void* stream, const float* x, int64_t rows, int64_t cols, float* mean, float* std);
/* StandardScaler fit, two passes with float64 accumulators (sklearn _incremental_mean_and_var):
 *   pass 1: sum[c] = sum_i x[i][c];  pass 2: corr[c] = sum_i (x - mean), m2[c] = sum_i (x - mean)^2
 * (all-reduce the outputs of each pass across ranks for a distributed fit). */
int64_t hlmc_colstats_workspace(int64_t n, int64_t cols);
int hlmc_colstats_sum(void* stream, const float* x, int64_t n, int64_t cols, double* sum, void* ws);
int hlmc_colstats_centered(void* stream, const float* x, int64_t n, int64_t cols, const double* mean, double* corr,
                           double* m2, void* ws);
/* StandardScaler.transform: y = f32(f32(x - mean) / scale) evaluated in float64; out dtype f32 or bf16 */
int hlmc_zscore_apply(void* stream, const float* x, int64_t n, int64_t cols, const double* mean, const double* scale,
                      int out_dtype, void* out);

/* ============================================================== VAE engine
 * Replaces the nn.Module forward/backward of
 *   HybridVAE        src/Convolutional_VAE.py:75-185   (kind 0; cfg = {latent, text_dim (0 = audio-only), H, W})
 *   ConditionalVAE   src/Conditional_VAE.py:109-231    (kind 1; cfg = {latent, text_dim, num_classes, H, W})
 *   VAE (Simple)     src/Simple_VAE.py:47-105          (kind 2; cfg = {input_dim, latent, n_hidden, h_1..h_n})
 *   SimpleAutoencoder src/Conditional_VAE.py:252-273   (kind 3; cfg = {input_dim, latent_dim}; see below)
 * and the torch train step of src/Convolutional_VAE.py:224-240.  Parameters are bound in the
 * reference's registration order (hlmc_net_param_info) as fp32 "master" tensors; dtype selects the
 * activation / MFMA operand type (HLMC_F32 exact fp32 MFMA, HLMC_BF16 bf16 MFMA with fp32 accumulate). */
typedef struct hlmc_net hlmc_net;
enum hlmc_net_kind { HLMC_NET_HYBRID = 0, HLMC_NET_CVAE = 1, HLMC_NET_SIMPLE = 2, HLMC_NET_AE = 3 };
/* Kind 3, the deterministic autoencoder baseline: Linear(D, 1024) - ReLU - Linear(1024, 256) - ReLU - Linear(256, L)
 * and its mirror, no BatchNorm (hlmc_net_num_bn = 0), no sampling; any input_dim, latent_dim >= 1.  Parameters:
 * encoder.0 / 2 / 4 then decoder.0 / 2 / 4, weight then bias.  Every entry point below takes it with these rules:
 *   hlmc_net_forward   in0 = x [B][input_dim]; recon [B][input_dim]; z (nullable) [B][latent_dim] = encoder(x);
 *                      in1, in2, eps, dropout, recon_text, mu, logvar must be NULL.  Train mode accepts B = 1.
 *   hlmc_net_encode    mu receives z; in1, in2 and logvar must be NULL.
 *   hlmc_net_decode    recon = decoder(z); cond, dropout and recon_text must be NULL.
 *   hlmc_net_backward  d_recon [B][input_dim]; d_mu (nullable) [B][latent_dim] is the upstream gradient of z, added
 *                      to the gradient that arrives at encoder.4's output from the decoder; d_logvar and d_recon_text
 *                      must be NULL.  One gradient bucket.
 * A violated rule returns HLMC_EINVAL before anything is launched. */

int hlmc_net_create(int kind, const int64_t* cfg, int ncfg, int dtype, hlmc_net** out);
int hlmc_net_destroy(hlmc_net* net);
int hlmc_net_num_params(const hlmc_net* net);
/* name (NUL-terminated, truncated to cap), ndim and shape (<= 4 dims) of parameter i */
int hlmc_net_param_info(const hlmc_net* net, int i, char* name, int cap, int* ndim, int64_t* shape);
/* float buffers: every BatchNorm's running_mean, running_var (in registration order);
 * num_batches_tracked (int64) is passed separately, one per BatchNorm */
int hlmc_net_num_bn(const hlmc_net* net);
int64_t hlmc_net_state_bytes(const hlmc_net* net);
int64_t hlmc_net_workspace_bytes(const hlmc_net* net, int64_t batch);
/* params / grads: arrays of num_params device pointers (fp32); running: 2*num_bn device pointers
 * (mean, var per BN); nbt: num_bn device int64 pointers; state: hlmc_net_state_bytes of device memory */
int hlmc_net_bind(hlmc_net* net, float* const* params, float* const* grads, float* const* running,
                  int64_t* const* nbt, void* state);
/* Forward.  train!=0: BatchNorm batch statistics (running stats updated), dropout mask applied (Simple);
 * eps [batch][latent] is the reparameterisation noise (torch.randn_like in the reference); eps = NULL draws it on
 * the device from the net's Philox4x32-10 stream (hlmc_net_set_rng; no host launch), kept for the backward.
 * in0 is read again by hlmc_net_backward (the first conv's weight gradient): it must stay allocated and unchanged
 * until then (stream order).
 * hybrid/cvae: in0 = audio [B][1][H][W], in1 = text [B][text_dim], in2 = condition [B][C] (cvae);
 * simple: in0 = x [B][input_dim], dropout = uint8 keep-mask per hidden unit (NULL = no dropout).
 * outputs: recon [B][...], recon_text [B][text_dim] (hybrid with text, cvae), mu, logvar [B][latent],
 * z [B][latent] (simple; nullable elsewhere).  Saves activations in ws for hlmc_net_backward. */
int hlmc_net_forward(hlmc_net* net, void* stream, int64_t batch, int train, const float* in0, const float* in1,
                     const float* in2, const float* eps, const uint8_t* dropout, float* recon, float* recon_text,
                     float* mu, float* logvar, float* z, void* ws);
/* Device reparameterisation noise (replaces torch.randn_like, src/Convolutional_VAE.py:162-165): the stream is
 * Philox4x32-10 keyed by `seed`; element g is component g % 4 of the block at counter g / 4, mapped by Box-Muller.
 * set_rng positions a net's stream (offset % 4 == 0); every forward drawing its own eps advances it by
 * round4(batch * latent).  hlmc_randn writes elements offset .. offset + n - 1 of stream `seed` to out. */
int hlmc_net_set_rng(hlmc_net* net, uint64_t seed, uint64_t offset);
int hlmc_net_get_rng(const hlmc_net* net, uint64_t* seed, uint64_t* offset);
int hlmc_randn(void* stream, float* out, int64_t n, uint64_t seed, uint64_t offset);
/* Device dropout stream (replaces the nn.Dropout(0.2) draws of src/Simple_VAE.py:57-61; as with eps, the values are
 * not a parity contract, any Bernoulli(0.8) stream serves).
 *
 * hlmc_dropout_mask: out[i] (uint8) = 1 (keep) or 0 for i in [0, n), decided by element g = offset + i of the
 * Philox4x32-10 stream `seed` hlmc_randn defines: the raw 32-bit word, component g % 4 of the block at counter
 * {g / 4 as 64 bits, 0, 0}, key {seed low, seed high}.  Keep iff word >= T, T = ceil(p_drop * 2^32) computed on the
 * host in double (858993460 for 0.2; 0 for p_drop = 0: every element kept).  An integer compare: no float conversion,
 * so a host restatement is exact.  One thread per Philox block writes its four bytes as one 32-bit store where
 * out + i is 4-aligned and as bytes otherwise (an unaligned out, the n % 4 tail); nothing outside [out, out + n) is
 * written.  No atomics, no scratch, the same bytes from run to run.  Checked on the host before any launch: out
 * non-NULL, n >= 0 (0 launches nothing), offset % 4 == 0, 0 <= p_drop < 1; else HLMC_EINVAL.
 *
 * hlmc_net_set_dropout_rng / hlmc_net_get_dropout_rng (Simple kind only, HLMC_EUNSUP otherwise; offset % 4 == 0): a
 * net's dropout stream, off when the net is created.  While off nothing changes: dropout == NULL in train mode means no
 * dropout.  While on, a train-mode hlmc_net_forward or hlmc_net_decode with dropout == NULL fills the workspace's mask
 * (batch * sum of the 2 n hidden widths bytes: the encoder blocks' [batch][width] masks, then the decoder blocks')
 * with one hlmc_dropout_mask launch at p_drop = 0.2 from the net's offset, and advances the offset by that byte count
 * rounded up to a multiple of 4; hlmc_net_backward reads the mask from the workspace as for a caller's mask.  An explicit
 * mask is used as before and does not advance the stream; eval mode and hlmc_net_encode draw nothing.  A train-mode
 * hlmc_net_encode therefore runs its encoder blocks WITHOUT dropout even while the stream is on (it takes no mask
 * argument either), unlike the encoder half of a train-mode hlmc_net_forward.  The offset is host-side state passed to
 * the launch by value: a call recorded into a HIP graph would replay one fixed mask, so callers that capture a step pass
 * an explicit mask (train.py and models.py do). */
int hlmc_dropout_mask(void* stream, uint8_t* out, int64_t n, double p_drop, uint64_t seed, uint64_t offset);
int hlmc_net_set_dropout_rng(hlmc_net* net, int on, uint64_t seed, uint64_t offset);
int hlmc_net_get_dropout_rng(const hlmc_net* net, int* on, uint64_t* seed, uint64_t* offset);
/* encoder only (latent extraction, src/Convolutional_VAE.py:286-303): mu, logvar */
int hlmc_net_encode(hlmc_net* net, void* stream, int64_t batch, int train, const float* in0, const float* in1,
                    const float* in2, float* mu, float* logvar, void* ws);
/* decoder only: HybridVAE.decode(z) (src/Convolutional_VAE.py:167-179), ConditionalVAE.decode(z, condition)
 * (src/Conditional_VAE.py:206-225), VAE.decode(z) (src/Simple_VAE.py:95-96).  z [B][latent]; cond [B][C]
 * (cvae, else NULL); dropout: the forward's keep-mask layout (Simple, train; only the decoder blocks' part is
 * read; NULL = none).  train != 0: decoder BatchNorms use batch statistics and update running stats.
 * recon [B][...], recon_text [B][text_dim] (hybrid with text, cvae; else NULL).  Inference only: a later
 * hlmc_net_backward needs a full hlmc_net_forward. */
int hlmc_net_decode(hlmc_net* net, void* stream, int64_t batch, int train, const float* z, const float* cond,
                    const uint8_t* dropout, float* recon, float* recon_text, void* ws);
/* Backward of the last hlmc_net_forward (same ws): writes (overwrites) all parameter gradients.
 * d_recon_text may be NULL when the model has no text branch. */
int hlmc_net_backward(hlmc_net* net, void* stream, int64_t batch, const float* d_recon, const float* d_recon_text,
                      const float* d_mu, const float* d_logvar, void* ws);

/* torch.optim.Adam step over every bound parameter (exp_avg / exp_avg_sq: num_params device pointers),
 * refreshing the packed GEMM weight layouts in the same pass. */
int hlmc_net_adam_step(hlmc_net* net, void* stream, float* const* exp_avg, float* const* exp_avg_sq, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step);
/* The same step with its step-dependent coefficients read from device memory (coef_dev: 6 floats written by
 * hlmc_adam_coef on the host and copied before each launch) — the form a captured HIP graph replays. */
int hlmc_net_adam_step_dev(hlmc_net* net, void* stream, float* const* exp_avg, float* const* exp_avg_sq,
                           const float* coef_dev);
/* torch.optim.Adam step coefficients for `step` (host): {b1, b2, eps, wd, lr/(1-b1^step), sqrt(1-b2^step)}. */
int hlmc_adam_coef(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* out6);
/* trust != 0: forward re-packs weights only when they changed through hlmc_net_adam_step (a caller that
 * writes parameters any other way must pass 0, the default, so forward always re-packs). */
int hlmc_net_set_trust_packs(hlmc_net* net, int trust);

/* enable != 0 (single process): hlmc_net_backward returns with the last weight gradients (encoder layers
 * 0-1) still in flight on the engine's weight-gradient stream, and the next hlmc_net_adam_step(_dev) updates
 * every other parameter first, then waits for them (Adam overlaps the tail of the backward pass).  Those
 * gradients are final only after that Adam step (or the next forward / backward, which wait for them).
 * Ignored while bucket sync is enabled. */
int hlmc_net_set_overlap_adam(hlmc_net* net, int enable);
/* Make every gradient of the last hlmc_net_backward final on `stream` (joins a pending tail; no-op otherwise). */
int hlmc_net_settle(hlmc_net* net, void* stream);

/* Data-parallel gradient buckets (the reference trains on one device; its DDP counterpart is the gradient
 * all-reduce of SURVEY.md §8e).  Bucket k = parameters [starts[k], starts[k-1]) in registration order
 * (starts[-1] = num_params), listed in the order hlmc_net_backward finishes them; the last start is 0.
 * Returns the bucket count (<= cap entries written) or a negative status. */
int hlmc_net_grad_buckets(const hlmc_net* net, int* starts, int cap);
/* enable != 0: every later hlmc_net_backward records one event per bucket once all of its gradients are
 * written (backward internally runs weight gradients on a second stream). */
int hlmc_net_set_bucket_sync(hlmc_net* net, int enable);
/* Make `stream` wait until bucket k of the last hlmc_net_backward is final (enqueue-only, no host sync). */
int hlmc_net_bucket_wait(hlmc_net* net, int k, void* stream);

/* ============================================================== live kernel timing (measurement only)
 * Arm: launches of the op kinds in `mask` (1 conv_s2 GEMM, 2 sub-pixel GEMM, 4 conv weight-gradient GEMM,
 * 8 linear GEMM, 16 linear weight-gradient GEMM, 32 STFT-mel, 64 BatchNorm / reduction streaming family) are
 * bracketed by HIP events on their launch
 * stream (up to max_launches; their algorithmic flops / bytes are summed).  Read: synchronises on the last
 * event, returns the count, the summed kernel time and work (and per-launch ms into ms_each[cap_each]), and
 * disarms.  bench.py uses this for the roofline of its dominant kernel inside the timed region. */
int hlmc_probe_arm(int mask, int max_launches);
int hlmc_probe_read(int* launches, double* total_ms, double* flops, double* bytes, float* ms_each, int cap_each);

/* ============================================================== losses
 * loss_function (src/Convolutional_VAE.py:187-194), cvae_loss_function (src/Conditional_VAE.py:233-246),
 * vae_loss (src/Simple_VAE.py:108-114).  sums3 (device, double[3]) receives
 *   { sum (ra-a)^2, sum (rt-t)^2, sum (1 + lv - mu^2 - exp lv) }; the caller forms the reference's tuple. */
int hlmc_loss_sums(void* stream, const float* ra, const float* a, int64_t na, const float* rt, const float* t,
                   int64_t nt, const float* mu, const float* lv, int64_t nl, double* sums3, void* ws);
int64_t hlmc_loss_workspace(int64_t na, int64_t nt, int64_t nl);
/* coef (DEVICE float[3]) = {ca, ct, ck}:  d ra = ca (ra - a), d rt = ct (rt - t), d mu = ck mu,
 * d lv = -0.5 ck (1 - exp lv).  For the summed hybrid loss with upstream grads (gT, gA, gX, gK) of
 * (total, l_audio, l_text, kld): ca = 2 (gT + gA), ct = 2 (w_text gT + gX), ck = beta gT + gK. */
int hlmc_loss_backward(void* stream, const float* ra, const float* a, int64_t na, float* dra, const float* rt,
                       const float* t, int64_t nt, float* drt, const float* mu, const float* lv, int64_t nl,
                       const float* coef, float* dmu, float* dlv);
/* hlmc_loss_sums and hlmc_loss_backward in one pass over the inputs (same outputs; the gradient does not
 * depend on the sums).  Used by the fused train step; ws as for hlmc_loss_sums. */
int hlmc_loss_sums_backward(void* stream, const float* ra, const float* a, int64_t na, float* dra, const float* rt,
                            const float* t, int64_t nt, float* drt, const float* mu, const float* lv, int64_t nl,
                            const float* coef, float* dmu, float* dlv, double* sums3, void* ws);

/* ============================================================== autoencoder train step: feed and loss
 * The loop of src/Conditional_VAE.py:428-452 -- DataLoader(batch_size=32, shuffle=True), mse_loss, Adam -- as one
 * captured graph replayed per step: hlmc_batch_gather, launched outside the graph with per-step arguments, fills the
 * graph's static input buffer, and hlmc_mse_rows inside the graph reads the row count from device memory, so the short
 * last batch of an epoch (padded with zero rows) needs no second graph.  Both allocate nothing, never synchronise and
 * use no floating-point atomics (the same bits from run to run).
 *
 * hlmc_batch_gather: out [B][d] f32 = rows X[idx[b]] for b < count, zero rows for count <= b < B; valid_dev (device
 * int32[1]) = count.  X [n][d] f32; idx: DEVICE int64 pointer to this step's count row indices; 1 <= count <= B.  An
 * index outside [0, n) is never dereferenced: its row is written as zeros and bit 1 of the device status word
 * (hlmc_device_status) is raised.
 *
 * hlmc_mse_rows: torch.nn.functional.mse_loss(recon[:valid], target[:valid]) and its gradient in one pass over the
 * dense [B][d] f32 arrays, valid = *valid_dev clamped to [0, B], read on the device.
 *   d_recon[b][j] = (float)(((double)recon - (double)target) * (2.0 / (valid d))) for b < valid, +0.0f for the other
 *                   rows whatever recon holds there (NaN included);
 *   sums2 (double[2]) = { sum over the valid rows of ((double)recon - (double)target)^2, valid d };
 *   acc (nullable, double[1]) += sums2[0] / sums2[1] (a running loss; unchanged when valid = 0).
 * The squared differences are added in float64 in a fixed order that depends on B and d alone: up to 16384 elements
 * one block of 1024 threads (thread t takes the float4 units t, t + 1024, ... in order, then the xor butterfly
 * 32, 16, .., 1 per wave and once more over the waves' totals), above that ceil(B d / 8192) <= 1024 such blocks and a
 * second launch that adds their totals the same way.  ws: hlmc_mse_rows_workspace(B, d) bytes (0: out of range),
 * non-decreasing in B and d. */
int hlmc_batch_gather(void* stream, const float* X, int64_t n, int d, const int64_t* idx, int count, int B, float* out,
                      int32_t* valid_dev);
int64_t hlmc_mse_rows_workspace(int64_t B, int64_t d);
int hlmc_mse_rows(void* stream, const float* recon, const float* target, int B, int d, const int32_t* valid_dev,
                  float* d_recon, double* sums2, double* acc, void* ws);

/* ============================================================== Simple VAE fit: epoch losses
 * The epoch means of src/Simple_VAE.py:190-196 without a read-back per step.  Step k of the epoch wrote its loss sums
 * (hlmc_loss_sums_backward) to sums[k] (DEVICE double[nb][3]); na_nl (DEVICE int64[nb][2]) holds each step's element
 * counts {batch * input_dim, batch * latent} (the short last batch has its own).  One launch, one thread, float64, in
 * step order, every operation rounded once (no FMA contraction):
 *   recon_k = sums[k][0] / na_k,  kl_k = -0.5 * sums[k][2] / nl_k,  total_k = recon_k + beta * kl_k,
 *   out3 (DEVICE double[3]) = { sum total_k / nb, sum recon_k / nb, sum kl_k / nb }.
 * The reference adds the float32 .item() of each step's loss; these are the float64 values of the same steps, about
 * 1e-7 relative apart.  Host checks: pointers non-NULL, nb >= 1, beta not NaN; else HLMC_EINVAL before any launch. */
int hlmc_vae_epoch_means(void* stream, const double* sums, const int64_t* na_nl, int nb, double beta, double* out3);

/* ============================================================== convolutional VAE fits: epoch totals
 * The epoch figures of src/Convolutional_VAE.py:237-256 and src/Conditional_VAE.py:331-345 without a read-back per step
 * or per validation batch.  Training step k of the epoch wrote its loss sums (hlmc_loss_sums_backward) to train_sums[k]
 * (DEVICE double[nt][3]), validation batch j (hlmc_loss_sums) to val_sums[j] (DEVICE double[nv][3]); a row is
 * { sum (ra-a)^2, sum (rt-t)^2, sum (1 + lv - mu^2 - exp lv) }.  One launch, one thread, float64, rows in step order,
 * every operation rounded once (no FMA contraction), the association as written:
 *   kld_s = -0.5 * s[2],  total_s = (s[0] + text_weight * s[1]) + beta * kld_s,
 *   out5 (DEVICE double[5]) = { sum_train total_s / train_div, sum_train s[0] / train_div, sum_train s[1] / train_div,
 *                               sum_train kld_s / train_div, sum_val total_s / val_div }.
 * Divisors: the data-set lengths for the hybrid script (len(loader.dataset)), the batch counts for the CVAE script
 * (len(loader)).  The reference adds the float32 .item() of each step's loss; these are the float64 values of the same
 * steps, about 1e-7 relative apart.  Host checks: pointers non-NULL, nt >= 1, nv >= 1, both divisors > 0, none of the
 * four scalars NaN; else HLMC_EINVAL before any launch. */
int hlmc_fit_epoch_totals(void* stream, const double* train_sums, int nt, const double* val_sums, int nv,
                          double text_weight, double beta, double train_div, double val_div, double* out5);

/* ============================================================== optimizer
 * torch.optim.Adam(lr, betas, eps, weight_decay) step (src/Convolutional_VAE.py:208,235) over
 * n tensors in one launch.  ptr arrays are HOST arrays of device pointers. */
int hlmc_adam_step(void* stream, int n, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, void* scratch);
int64_t hlmc_adam_scratch_bytes(int n);

/* ============================================================== K-Means (sklearn semantics)
 * Device kernels under the Python KMeans host (src/Convolutional_VAE.py:317-319,
 * src/Conditional_VAE.py:293-295, :528; src/Simple_VAE.py:244-261).  X row-major float32 [n][d]. */
/* X_mean = sequential float32 column sums / n (numpy mean(axis=0) order); Xc = X - X_mean;
 * var (nullable) = np.var(X, axis=0) in the same order (sklearn's tolerance input) */
int hlmc_km_center(void* stream, const float* X, int64_t n, int d, float* mean, float* var, float* Xc);
/* out[t][i] = float32(max(0, ||x_c||^2 - 2 x_c.x_i + ||x_i||^2)) evaluated in float64, c = cand[t]
 * (cand is a HOST array of ncand <= 16 row indices) — sklearn _euclidean_distances_upcast */
int hlmc_km_sqdist_rows(void* stream, const float* X, int64_t n, int d, const int64_t* cand, int ncand, float* out);
/* E-step: labels[i] = argmin_j (||c_j||^2 + (-2) x_i.c_j) (float32, first minimum);
 * n_changed (device int32) += count(labels != labels_old) when labels_old != NULL */
int hlmc_km_assign(void* stream, const float* X, int64_t n, int d, const float* centers, int k, int32_t* labels,
                   const int32_t* labels_old, int32_t* n_changed);
/* M-step sums in index order (float32, as sklearn's single-thread loop): sums [k][d], weight [k] */
int hlmc_km_sums(void* stream, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sums,
                 float* weight);
/* The same sums through a stable partition of the rows by label (device workspace of
 * hlmc_km_sums_workspace(n, k) bytes): the rows of each cluster become one contiguous list in row order and
 * one 1024-thread block per (64-column slab, cluster) runs a loader/adder ring: 15 loader waves gather 64-row
 * chunks into an 8-slot LDS ring, one adder wave adds them in row order.  Limits: 0 < n < 2^30, k <= 8192.
 * n <= 4096 rows take hlmc_km_sums instead (one launch is faster there); the results are the same bits. */
int64_t hlmc_km_sums_workspace(int64_t n, int k);
int hlmc_km_sums_part(void* stream, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sums,
                      float* weight, void* ws, int64_t ws_bytes);
/* per-row ||x_i - c_{l_i}||^2 in sklearn's _euclidean_dense_dense float32 order -> out [n] */
int hlmc_km_rowdist(void* stream, const float* X, int64_t n, int d, const float* centers, const int32_t* labels,
                    float* out);
/* sum of the row distances accumulated sequentially in float32 (sklearn _inertia_dense) -> out[0]; tmp [n] */
int hlmc_km_inertia(void* stream, const float* X, int64_t n, int d, const float* centers, const int32_t* labels,
                    float* out, float* tmp);

/* ---- R <= 64 restarts (n_init) in lockstep: the same arithmetic per restart, one launch per stage for all.
 * Restart r's centres are centers + r*k*d, its labels labels + r*n; `active` is a bitmask of the restarts a launch
 * runs (the others are left untouched).  The restarts of KMeans(n_init=10) share X and are independent objects. */
int hlmc_km_assign_batch(void* stream, const float* X, int64_t n, int d, const float* centers, int k, int R,
                         uint64_t active, int32_t* labels, const int32_t* labels_old, int32_t* n_changed);
/* hlmc_km_sums_part per restart; ws: R * hlmc_km_sums_workspace(n, k) bytes; sums [R][k][d], weight [R][k] */
int hlmc_km_sums_batch(void* stream, const float* X, int64_t n, int d, const int32_t* labels, int k, int R,
                       uint64_t active, float* sums, float* weight, void* ws, int64_t ws_bytes);
/* Lloyd centre update (sklearn: centers_new *= 1 / weight_in_clusters, reciprocal in double):
 * C_new[r][j] = sums[r][j] * (float)(1.0 / weight[r][j]); info[r][j] (j < k) = ||C_new[r][j] - C_old[r][j]||^2 in
 * _euclidean_dense_dense float32 order, info[r][k] = 1 when a cluster of restart r is empty (nothing else is written
 * for it: the host relocates, sklearn _relocate_empty_clusters_dense), else 0.  info: [R][k + 1] floats */
int hlmc_km_update_batch(void* stream, int k, int d, int R, uint64_t active, const float* sums, const float* weight,
                         const float* C_old, float* C_new, float* info);
/* k-means++ candidate draw of every restart (sklearn _kmeans_plusplus): restart r's closest distances are the row
 * prev + (r*prevT + best[r])*n; cand[r][t] = min(searchsorted(np.cumsum(closest, dtype=float64), rvals[r][t]), n-1)
 * from a parallel float64 prefix with a rigorous error bracket around numpy's sequential cumsum; amb[r][t] = 1 where
 * the bracket cannot decide (the caller redoes that trial with numpy; rvals within ~1e-11 relative of a prefix).
 * best, rvals: HOST arrays [R], [R*T]; cand (int64), amb (int32): device [R*T]; R*T <= 64 */
int hlmc_km_pp_search(void* stream, int64_t n, int R, int T, const float* prev, int prevT, const int32_t* best,
                      const double* rvals, int64_t* cand, int32_t* amb);
/* out[r][t][i] = min(closest_r[i], sqdist(X[cand[r][t]], X[i])) (hlmc_km_sqdist_rows arithmetic, candidates from the
 * DEVICE array cand [R*T]); prev == NULL: the plain distances (first centre), else closest_r as in hlmc_km_pp_search */
int hlmc_km_pp_dist(void* stream, const float* X, int64_t n, int d, int R, int T, const int64_t* cand, const float* prev,
                    int prevT, const int32_t* best, float* out);
/* hlmc_km_inertia per restart: out [R], tmp [R][n] */
int hlmc_km_inertia_batch(void* stream, const float* X, int64_t n, int d, const float* centers, int k,
                          const int32_t* labels, int R, float* out, float* tmp);

/* ============================================================== cluster-quality metrics
 * sklearn.metrics.silhouette_score / silhouette_samples (metric "euclidean"), replacing the calls at
 * src/Convolutional_VAE.py:320,337,361,399, src/Conditional_VAE.py:298, src/Simple_VAE.py:247,256,262.
 * X [n][d] f32 (n >= 2, 1 <= d <= 128), 2 <= k <= n - 1 (sklearn's range; k above the 64 -- 62 for d > 64 --
 * accumulator rows LDS holds takes one distance launch per label window).  samples (nullable) [n] f64, score: device
 * f64 scalar.  Deterministic (fixed-order f64 reductions).
 * PRECONDITION (both entry points): labels are int32 in [0, k).  Sizes, pointers and the workspace size are checked on
 * the host; label VALUES are not: the kernels index the counts, the centroids and LDS with them unchecked (the Python
 * wrappers encode labels with np.unique, which guarantees it).
 * Distances are float32 sums of squared direct differences (no Gram form), float32 sqrt, summed in float64.
 * Workspace of hlmc_silhouette (bytes; r256 = round up to 256):
 *   [0, 8 n k)                 S [n][k] f64, S[i][c] = sum over rows j with label c of ||x_i - x_j||
 *   [r256(8 n k), + r256(4 k)) counts [k] int32 (rows per label)
 *   then 512 f64               block partial sums of the coefficients */
int64_t hlmc_silhouette_workspace(int64_t n, int k);
int hlmc_silhouette(void* stream, const float* X, int64_t n, int d, const int32_t* labels, int k, double* samples,
                    double* score, void* ws, int64_t ws_bytes);
/* M labellings of the same X in one distance pass: the K-Means, Ward and DBSCAN parameter searches of
 * src/Convolutional_VAE.py:311-374 score up to 43 labellings of one latent matrix.  labels: device [M][n] int32, row m
 * in [0, ks[m]); ks: HOST array [M]; samples (nullable): device [M][n] f64; scores: device [M] f64.  1 <= M <= 64,
 * every ks[m] in [2, n - 1], n and d as above, and K n 8 bytes must not overflow (else -1 / HLMC_EINVAL).  Label VALUES
 * are an unchecked precondition, as above.
 * The labellings form one concatenated label space of K = sum ks[m] columns; labelling m owns the columns
 * [off_m, off_m + ks[m]), off_m = ks[0] + ... + ks[m - 1].  The distance kernel walks windows of 64 columns (58 for
 * d > 64: what 160 KB of LDS hold next to the X tile and the labels of the up to kw / 2 + 1 labellings a window of kw
 * columns overlaps); a labelling may straddle two windows; ||x_i - x_j|| is computed once per window that has j's
 * label of some labelling inside.  For every labelling m, S[:, off_m : off_m + ks[m]], its counts, samples and score
 * are bit-identical to hlmc_silhouette on that labelling alone (same per-thread summation order, same arithmetic).
 * Workspace of hlmc_silhouette_batch (bytes; r256 = round up to 256):
 *   [0, 8 n K)                 S [n][K] f64, S[i][off_m + c] = sum over rows j with label c in labelling m of ||x_i - x_j||
 *   [r256(8 n K), + r256(4 K)) counts [K] int32, counts[off_m + c] = rows with label c in labelling m
 *   then M x 512 f64           block partial sums of the coefficients, labelling m at [512 m, 512 m + 512) */
int64_t hlmc_silhouette_batch_workspace(int64_t n, const int32_t* ks, int M);
int hlmc_silhouette_batch(void* stream, const float* X, int64_t n, int d, const int32_t* labels, const int32_t* ks, int M,
                          double* samples, double* scores, void* ws, int64_t ws_bytes);
/* out2 (device f64[2]) = { davies_bouldin_score, calinski_harabasz_score } (src/Convolutional_VAE.py:400,
 * src/Simple_VAE.py:257,263), sklearn 1.7 branches included (a centroid distance of 0 contributes 0; all intra
 * distances or all centroid distances within 1e-8 of 0 -> Davies-Bouldin 0; zero intra dispersion -> Calinski-Harabasz
 * 1).  n >= 2, 1 <= d <= 4096, 2 <= k <= min(n - 1, 1024); labels as above, and every label in [0, k) must occur.
 * All accumulation in float64, fixed order.  Workspace (f64 units unless stated, in this order):
 *   part [64][k][d]   per row block: sum of the block's rows of each label
 *   part2 [64][k][2]  per row block: sum of ||x - cent|| and of ||x - cent||^2 of each label
 *   cent [k][d]       centroids;   mean [d]  grand mean
 *   counts [k] int32  padded to a multiple of 256 bytes
 *   intra [k]         mean distance of a label's rows to its centroid */
int64_t hlmc_cluster_scores_workspace(int k, int d);
int hlmc_cluster_scores(void* stream, const float* X, int64_t n, int d, const int32_t* labels, int k, double* out2,
                        void* ws, int64_t ws_bytes);

/* ============================================================== DBSCAN
 * sklearn.cluster.DBSCAN(eps, min_samples=5).fit_predict(latent_matrix) at src/Convolutional_VAE.py:353-354,382
 * (float32 input, brute-force neighbourhoods), labels and core samples bit-identical to sklearn 1.7.
 *
 * hlmc_dbscan_neighbors: one pass over the fp64 (MFMA) distance tiles for E <= 32 squared radii.  i and j are
 * neighbours for radius e iff max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) <= radii_sq[e], all in float64 on the float32
 * rows.  radii_sq is a HOST array; for sklearn's float32 path pass (double)((float)eps * (float)eps).  Writes the
 * bit-packed adjacency [E][n][ceil(n/64)] into the workspace, counts [E][n] int32 (neighbours of each row, self
 * included) and borderline [E] uint64: pairs i < j with |d^2 - r| <= 4 (d + 4) 2^-53 (|x_i|^2 + |x_j|^2), the only
 * ones another summation order could decide differently.  X [n][d] f32, 1 <= n <= 262144, d >= 1.
 *
 * hlmc_dbscan_labels: labels of radius e from the adjacency a preceding hlmc_dbscan_neighbors call (same n, E,
 * workspace) left behind.  core [n] uint8 = (counts >= min_samples); clusters are the connected components of
 * the core-core graph numbered by their smallest core index; a border point takes the smallest cluster number
 * among its core neighbours; noise is -1.  n_clusters (nullable): device int32 scalar.  No host
 * synchronisation, integer atomics only, deterministic. */
int64_t hlmc_dbscan_workspace(int64_t n, int E);   /* bytes; 0 when n or E is out of range */
int hlmc_dbscan_neighbors(void* stream, const float* X, int64_t n, int d, const double* radii_sq, int E, int32_t* counts,
                          uint64_t* borderline, void* ws, int64_t ws_bytes);
int hlmc_dbscan_labels(void* stream, int64_t n, int E, int e, int min_samples, const int32_t* counts, void* ws,
                       int64_t ws_bytes, int32_t* labels, uint8_t* core, int32_t* n_clusters);

/* ---- Ward agglomerative clustering --------------------------------------------------------------------------------
 * sklearn.cluster.AgglomerativeClustering(n_clusters=k).fit_predict(latent_matrix) at src/Convolutional_VAE.py:334-342,
 * 381 (Ward linkage, no connectivity = scipy.cluster.hierarchy.ward on the float64-upcast rows).  2 <= n <= 32768
 * (the distance matrix is n * n * 8 bytes, 8 GiB at the cap), d >= 1.
 *
 * hlmc_ward_pdist: D [n][n] float64, full and symmetric with a zero diagonal, row-major.  D[i][j] = sqrt(s) with
 * s = 0 and then, for k = 0 .. d-1 in that order, t = x_ik - x_jk, s = s + t * t in float64 without FMA: scipy's pdist
 * bit for bit.  X [n][d] f32.
 *
 * hlmc_ward_chain: the nearest-neighbour chain on D (which it destroys), n - 1 merges, one launch of one workgroup.
 * An empty chain starts at the lowest live index; from the chain top x the scan starts at the predecessor and takes
 * a live i != x only when D[x][i] is strictly smaller (ties: the predecessor first, then the lowest index).  Merge m
 * in merge order (NOT sorted by height): merge_a[m] < merge_b[m] the two representatives (a dies, b carries the
 * merged cluster), merge_dist[m] their distance, merge_size[m] the merged point count; all four are device arrays of
 * n - 1 elements.  Distances to the merged cluster follow Lance-Williams for Ward, left to right without FMA:
 *   t = 1.0 / (double)(ni + nx + ny)
 *   sqrt(((ni + nx) * t) * dxi * dxi + ((ni + ny) * t) * dyi * dyi - (ni * t) * dxy * dxy)
 * Workspace (hlmc_ward_workspace bytes): [D: n * n * 8 rounded up to 256][int32 status, 256 bytes][int32 chain[n]].
 * The size includes room for D so that one allocation serves both stages (pass D = ws); D may also live elsewhere.
 * The status word is 0 after a complete run, 1 when a scan found no neighbour (NaN or +inf in D), 2 when a loop
 * bound computed from n was exhausted; the kernel then stops, and the call returns HLMC_EDEVICE.  The call copies
 * the status word back and so synchronises the stream: the merge records are complete when it returns. */
int64_t hlmc_ward_workspace(int64_t n);            /* bytes incl. D; 0 when n is out of range */
int hlmc_ward_pdist(void* stream, const float* X, int64_t n, int d, double* D);
int hlmc_ward_chain(void* stream, int64_t n, double* D /* in, destroyed */, int32_t* merge_a, int32_t* merge_b,
                    double* merge_dist, int32_t* merge_size, void* ws, int64_t ws_bytes);

/* ---- PCA ------------------------------------------------------------------------------------------------------------
 * sklearn.decomposition.PCA(n_components=k).fit_transform at src/Simple_VAE.py:258-263 (370 -> 32) and
 * src/Conditional_VAE.py:422-425 (290 -> 64): the two float64 GEMMs of the exact decomposition on the fp64 MFMA; the
 * d x d eigen-solve between them is the caller's (hlmc_amd.PCA runs numpy.linalg.eigh on the host).
 *
 * hlmc_pca_cov: mean [d] float64 and G [d][d] float64, row-major, full and symmetric bit for bit:
 *   mean_c = (sum_r x_rc) / n,   G[i][j] = sum_r ((double)x_ri - mean_i) ((double)x_rj - mean_j).
 * X [n][d] f32, 2 <= n <= 2^24, 1 <= d <= 1024.  The rows are cut into S = ceil(n / L) slabs of
 * L = max(256, ceil(n / 128) rounded up to a multiple of 32) rows (S <= 128, a function of n alone); every sum runs in
 * a fixed order and the slabs are added in slab order, so the result is bit-identical from run to run.
 * |G' - G|_ij <= (n + 8) 2^-53 sum_r |xc_ri| |xc_rj| + n |dm_i| |dm_j| with |dm_c| <= n 2^-53 mean_r |x_rc| the error
 * of the mean (assuming the MFMA rounds each product and each addition of its 4-step inner sum at most once).
 * Workspace (hlmc_pca_workspace bytes), T = ceil(d / 64) feature tiles, P = T (T + 1) / 2 tile pairs numbered row-major
 * over the upper triangle ((0,0) (0,1) .. (0,T-1) (1,1) ..):
 *   [colsum: float64 [S][d], the slabs' column sums, rounded up to 256 bytes]
 *   [part:   float64 [S][P][64][64], slab s's share of the tile (ti, tj): part[s][pair][i][j] belongs to
 *            G[64 ti + i][64 tj + j]; entries past d are 0, and of a diagonal pair only i <= j is used]
 * G[a][b] for a <= b is part[0] + part[1] + ... + part[S-1] of its entry, added in that order.
 *
 * hlmc_pca_project: out [n][q] f32, out[r][j] = (float)(sum_c ((double)A[r][c] - a_off[c]) B[c][j] + o_off[j]),
 * accumulated in float64 and rounded once.  A [n][p] f32, B [p][q] float64, a_off [p] and o_off [q] float64 or NULL
 * (= 0).  n >= 1 (below 2^31), 1 <= p, q <= 1024.  transform: a_off = mean, B = components^T; inverse_transform:
 * B = components, o_off = mean; whitening: a scaled B. */
int64_t hlmc_pca_workspace(int64_t n, int d);      /* bytes; 0 when n or d is out of range */
int hlmc_pca_cov(void* stream, const float* X, int64_t n, int d, double* mean, double* G, void* ws, int64_t ws_bytes);
int hlmc_pca_project(void* stream, const float* A, int64_t n, int p, const double* B, int q, const double* a_off,
                     const double* o_off, float* out);

/* ---- t-SNE ----------------------------------------------------------------------------------------------------------
 * sklearn.manifold.TSNE(n_components=2, random_state=42[, perplexity=30]).fit_transform(latents) at
 * src/Simple_VAE.py:302-303, src/Convolutional_VAE.py:468-469 and src/Conditional_VAE.py:515-517: the objective of
 * sklearn 1.7's method='barnes_hut' (sparse kNN affinities P, Student-t Q with one degree of freedom) with the
 * repulsive sum and Z taken over ALL pairs -- sklearn's angle = 0 -- in a fixed order.  No float atomics: two runs give
 * the same bits.  2 <= n <= 131072, 1 <= d <= 4096, 1 <= k <= min(512, n - 1); sklearn's k is
 * min(n - 1, int(3 perplexity + 1)).  One workspace of hlmc_tsne_workspace(n, d, k) bytes serves all four calls; the
 * gradient's part comes first and depends on n alone, so hlmc_tsne_gradient / hlmc_tsne_run accept the size of any
 * (d, k) of the same n.  No call synchronises with the host.
 *
 * hlmc_tsne_knn: nbr_idx [n][k] int32 and nbr_d2 [n][k] float64, the k nearest OTHER rows of each row of X [n][d] f32,
 * ascending by squared distance, equal distances by ascending index.  The distance is
 * max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) in float64 (the dot product on the fp64 MFMA),
 * |d2' - d2| <= 1.01 (d + 4) 2^-52 (|x_i|^2 + |x_j|^2) (oracle/kmeans_oracle.py sqdist_bound without its float32 term).
 *
 * hlmc_tsne_affinities: sklearn's _binary_search_perplexity per row in float64 on (double)(float)nbr_d2 (start beta = 1,
 * double / halve while a bound is infinite, <= 100 steps, |H - log((float)perplexity)| <= 1e-5, a zero sum becomes
 * (double)1e-8f): beta [n] float64 and cond_p [n][k] float64 in the neighbours' order.  A row's sums are taken by one wave: lane
 * l adds its neighbours l, l + 64, ... in that order, the lanes are combined by the xor butterfly 32, 16, .., 1.  Then
 * (P + P^T) / max(total, 2^-52) over the union pattern, without the entries whose sum is exactly 0 (an underflowed
 * exp; scipy's P + P.T drops them too), as a CSR matrix: indptr [n + 1] int64, indices int32 ascending
 * within each row, values float32; indices and values need room for 2 n k entries, indptr[n] are used.  Entry (i, j)
 * and entry (j, i) hold the same bits.  The total is added per row in column order, the rows' sums by
 * "thread t adds rows t, t + 256, ..., then the tree 128, 64, .., 1".
 *
 * hlmc_tsne_gradient: grad [n][2] f32 = 4 (exaggeration sum_j p_ij q_ij (y_i - y_j) - sum_{j != i} q_ij^2 (y_i - y_j) / Z),
 * q_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} q_ij: what sklearn's _kl_divergence_bh returns at angle = 0 for
 * P scaled by `exaggeration` (P is not rescaled in memory).  Y [n][2] f32.  stats [3] float64 (device):
 * stats[0] = Z always; with want_stats != 0 also stats[1] = sum over the stored entries of
 * p log(max(p, t) / max(q / Z, t)) with p = exaggeration * value and t = float32's smallest normal (sklearn's error
 * term), and stats[2] = |grad|_2 of the float32 gradient.
 * Repulsion: rows in blocks of 256 (one per thread), columns in S = ceil(n / L) slabs of
 * L = max(256, ceil(n / 64) rounded up to a multiple of 256) columns; the pair arithmetic is float32 without FMA
 * (dx = y_i0 - y_j0, dy likewise, q = rcp(1 + (dx dx + dy dy)), q q dx), every term is widened and added in float64 in
 * column order, the slabs' partials are added in slab order.  Attraction: one wave per row in float64, lane l takes the
 * stored entries l, l + 64, ..., then the xor butterfly.  Workspace, gradient part:
 *   [part:    float64 [S][3][n]: slab s's sums for row i, component 0 / 1 the repulsive force, 2 the sum of q]
 *   [rep:     float64 [3][n]: part[0] + part[1] + ... + part[S-1] in that order]
 *   [rowstat: float64 [2][n]: the rows' error terms | squared gradient norms]
 *   [grad:    float32 [n][2]: the gradient of hlmc_tsne_run's last iteration]
 * each rounded up to 256 bytes.
 *
 * hlmc_tsne_run: n_iter iterations of sklearn's _gradient_descent on (Y, update, gains), all [n][2] f32, in float32
 * without FMA: g = the gradient at Y; gains += 0.2 where update * g < 0, else gains *= 0.8; gains = max(gains, 0.01);
 * update = momentum * update - learning_rate * (g * gains); Y += update.  stats as above, of the LAST iteration's
 * gradient (taken at the Y before its update, as sklearn's error and gradient norm are). */
int64_t hlmc_tsne_workspace(int64_t n, int d, int k);   /* bytes; 0 when a size is out of range */
int hlmc_tsne_knn(void* stream, const float* X, int64_t n, int d, int k, int32_t* nbr_idx, double* nbr_d2, void* ws,
                  int64_t ws_bytes);
int hlmc_tsne_affinities(void* stream, const int32_t* nbr_idx, const double* nbr_d2, int64_t n, int k,
                         double perplexity, double* beta, double* cond_p, int64_t* indptr, int32_t* indices,
                         float* values, void* ws, int64_t ws_bytes);
int hlmc_tsne_gradient(void* stream, const float* Y, int64_t n, const int64_t* indptr, const int32_t* indices,
                       const float* values, double exaggeration, float* grad, double* stats, int want_stats, void* ws,
                       int64_t ws_bytes);
int hlmc_tsne_run(void* stream, float* Y, float* update, float* gains, int64_t n, const int64_t* indptr,
                  const int32_t* indices, const float* values, double exaggeration, double momentum,
                  double learning_rate, int n_iter, double* stats, void* ws, int64_t ws_bytes);


/* ============================================================== op-level entry points
 * The kernels hlmc_net_* is built from, on NHWC activations (dtype HLMC_F32 / HLMC_BF16 for x, y, packed
 * weights; bias / dW always f32).  ws = split-K scratch (>= 256 MiB is always enough at B <= 256).
 *   conv_s2   y[B,Hi/2,Wi/2,Co] = Conv2d(k3,s2,p1)(x[B,Hi,Wi,Ci]) + bias;  wp [Co][3][3][Ci]
 *   subpixel  y[B,2Hi,2Wi,Co]  = ConvTranspose2d(k3,s2,p1,op1)(x[B,Hi,Wi,Ci]) + bias; wp [Co][3][3][Ci]
 *             (w_torch[Ci][Co][kh][kw] -> wp[co][kh][kw][ci]; also the data gradient of conv_s2)
 *   wgrad_s2  dW[M][C][3][3] = sum_{b,r,c} L[b,r,c,m] Xh[b,2r-1+kh,2c-1+kw,ci]   (L [B,Hl,Wl,M], Xh [B,2Hl,2Wl,C])
 *   linear    y[m*ldy+n] (+)= act(sum_k x[m*ldx+k] w[n*ldw+k] + bias[n]), act 0 none / 1 relu
 *   linear_wgrad dW[n][k] = sum_b dy[b*lddy+n] x[b*ldx+k]
 *   conv_c1_s2 / convT_c1 / wgrad_c1: the single-channel first / last layers (f32 input image). */
int hlmc_op_conv_s2(void* stream, int dtype, const void* x, int B, int Hi, int Wi, int Ci, const void* wp,
                    const float* bias, int Co, void* y, void* ws, int64_t ws_bytes);
int hlmc_op_subpixel(void* stream, int dtype, const void* x, int B, int Hi, int Wi, int Ci, const void* wp,
                     const float* bias, int Co, void* y, void* ws, int64_t ws_bytes);
int hlmc_op_wgrad_s2(void* stream, int dtype, const void* L, int B, int Hl, int Wl, int M, const void* Xh, int C,
                     float* dW, void* ws, int64_t ws_bytes);
/* relu_ref (nullable, row stride ldy, act 0): y zeroed where relu_ref <= 0 after the accumulate (a dense layer's
 * data gradient with the ReLU backward of the layer below fused into the epilogue). */
int hlmc_op_linear(void* stream, int dtype, const void* x, int ldx, int M, int K, const void* w, int ldw,
                   const float* bias, int N, void* y, int ldy, int act, int accumulate, int out_f32, void* ws,
                   int64_t ws_bytes, const void* relu_ref);
/* db (nullable): the bias gradient sum_b dy[b][n], from the same GEMM (a virtual ones column on x). */
int hlmc_op_linear_wgrad(void* stream, int dtype, const void* dy, int lddy, const void* x, int ldx, int Mb, int N,
                         int K, float* dW, float* db, void* ws, int64_t ws_bytes);
int hlmc_op_conv_c1_s2(void* stream, int dtype, const float* x, int B, int Hi, int Wi, const float* w,
                       const float* bias, int Co, void* y);
int hlmc_op_convT_c1(void* stream, int dtype, const void* x, int B, int Hi, int Wi, int Ci, const float* w,
                     const float* bias, float* y);
int hlmc_op_wgrad_c1(void* stream, int dtype, const void* L, int B, int Hl, int Wl, int M, const float* Xh,
                     float* dW, void* ws, int64_t ws_bytes);
/* The train-mode forward of the LDS halo-tile conv (kind 0: conv_s2) / sub-pixel conv (kind 1: subpixel), bf16, at
 * the shapes where hlmc_net_forward runs them (conv Ci 32 -> Co 64 at Wi 64, Ci 64 -> 128 at Wi 32; sub-pixel
 * Ci 64 -> 32 at Wi 32, Ci 128 -> 64 at Wi 16), as the engine launches them:
 *   - out_sums (device f64 [2 Co]) = (sum_rows y | sum_rows y^2) of the stored bf16 output, from the epilogue's exact
 *     statistics accumulator (the next BatchNorm's batch statistics; src/Convolutional_VAE.py:80-100, 124-139);
 *   - gamma != NULL: x is the PRE-BatchNorm map of the layer below; its train-mode BatchNorm2d (batch statistics,
 *     biased variance, eps) + LeakyReLU(0.01) is applied while the input is staged.  mean_out / invstd_out [Ci]
 *     receive the batch statistics, running_mean / running_var / num_batches_tracked (nullable) are updated as
 *     torch does (momentum, unbiased variance), a_out [B,Hi,Wi,Ci] bf16 receives the activation.
 * ws: hlmc_op_halo_workspace(Ci, Co) bytes.  Returns an error for any other shape. */
/* Train-mode BatchNorm2d + LeakyReLU(0.01) backward of one layer (the engine's bn_act_bwd: the moments pass
 * [sum dz | sum dz * xhat] into an exact accumulator, then the apply pass dy = gamma invstd (dz - mean dz -
 * xhat mean(dz xhat)) with its conv-bias column sums), src/Convolutional_VAE.py:80-100 / 124-139 backward.
 * da / y / dy: [R][C] in `dtype` (bf16 or f32; da = grad of the activation, y = the pre-BN map); mean / invstd:
 * the forward batch statistics; dgamma / dbeta [C] (f32) written; dbias (nullable, f32 [C]) = column sums of the
 * stored dy.  ws: hlmc_op_bn_bwd_workspace(C) bytes (zeroed here). */
int64_t hlmc_op_bn_bwd_workspace(int C);
int hlmc_op_bn_bwd(void* stream, int dtype, const void* da, const void* y, int64_t R, int C, const float* mean,
                   const float* invstd, const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                   float* dbias, void* ws, int64_t ws_bytes);
/* hlmc_op_bn_bwd in its general form (bn_act_bwd as the dense and BatchNorm1d layers call it): act 0 LeakyReLU(0.01) /
 * 1 ReLU / 2 none; mask (nullable, dense [R][C] bytes): dz = da * (mask != 0) * mscale * act'(z), the Dropout behind
 * the activation; lda >= C: the row stride of da (y and dy are dense).  R >= 1.  With a mask the two-pass form always
 * runs; without one R <= 1024 runs the one-launch small-layer kernel.  ws: hlmc_op_bn_bwd_workspace(C) bytes. */
int hlmc_op_bn_act_bwd(void* stream, int dtype, const void* da, int lda, const void* y, int64_t R, int C,
                       const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                       const uint8_t* mask, float mscale, void* dy, float* dgamma, float* dbeta, float* dbias, void* ws,
                       int64_t ws_bytes);
/* BatchNorm forward of one [R][C] map y (dtype bf16 / f32), a = act(gamma (y - mean) invstd + beta) [* (mask != 0) *
 * mscale], act as above, as the engine launches it:
 *   mode 0  train: moments pass + the activation kernel that finalizes the statistics itself (C <= 512; wider: a
 *           finalize launch between them);
 *   mode 1  train: the same with the statistics delivered beforehand (a separate moments launch into the accumulator);
 *   mode 2  train statistics only (moments + finalize); gamma / beta / a unused;
 *   mode 3  eval: mean / invstd from running_mean / running_var (required), then the activation.
 * Train modes write mean_out / invstd_out [C] (biased variance), blend running_mean / running_var (nullable pair;
 * momentum, unbiased variance; R == 1: the biased value 0) and add 1 to num_batches_tracked (nullable).
 * a: row stride lda >= C (a multiple of 16 bytes); mask: dense [R][C] bytes.  flat_hw > 0: a is written NCHW-flat
 * instead, [R / flat_hw][flat_ld] with channel c of pixel p at column c * flat_hw + p (flat_ld >= C * flat_hw; no
 * mask; lda unused); flat_hw == flat_ld == 0: the NHWC rows.  out_sums (nullable, device f64 [2 C], train modes) =
 * (sum_rows y | sum_rows y^2) from the exact accumulator.  ws: hlmc_op_bn_fwd_workspace(C) bytes (zeroed here). */
int64_t hlmc_op_bn_fwd_workspace(int C);
int hlmc_op_bn_fwd(void* stream, int dtype, int mode, const void* y, int64_t R, int C, const float* gamma,
                   const float* beta, int act, const uint8_t* mask, float mscale, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* mean_out,
                   float* invstd_out, void* a, int lda, int flat_hw, int flat_ld, double* out_sums, void* ws,
                   int64_t ws_bytes);
/* hlmc_op_conv_c1_s2 (Co == 32) in the two forms that also reduce over its stored output y, as the engine runs them:
 *   mode 1 (the encoder's input conv): out_sums (device f64 [2 Co]) = (sum y | sum y^2), the next BatchNorm's batch
 *           statistics, from the kernel's exact accumulator;
 *   mode 2 (the data gradient of the decoder's output convT; y is then the gradient of the last BatchNorm + LeakyReLU
 *           layer's output, ybn [B, Hi/2, Wi/2, Co] that layer's pre-BN map with its mean / invstd / gamma / beta):
 *           out_sums = (sum dz | sum dz xhat), dz = y lrelu'(xhat gamma + beta).  With dy_out (nullable) the
 *           BatchNorm backward then runs its apply pass alone on those moments (no moments pass): dy_out (dtype),
 *           dgamma, dbeta [Co].
 * ws: hlmc_op_conv_c1_s2_fused_workspace(Co) bytes (zeroed here). */
int64_t hlmc_op_conv_c1_s2_fused_workspace(int Co);
int hlmc_op_conv_c1_s2_fused(void* stream, int dtype, int mode, const float* x, int B, int Hi, int Wi, const float* w,
                             const float* bias, int Co, void* y, double* out_sums, const void* ybn, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, void* dy_out, float* dgamma,
                             float* dbeta, void* ws, int64_t ws_bytes);
/* The latent layers' GEMMs whose split-K reduce launch carries the next step's arithmetic.  x [B][ldx] and the weight
 * w [N][ldw] (N rows of K) in dtype; S_out (nullable, host) receives the split count.  ws: hlmc_op_latent_workspace
 * bytes (one size serves the three entries at the same B, K, L).
 *   heads_reparam       w = fc_mu's L rows, then fc_logvar's: mu / lv [B][L] f32 = x w^T + bias, copies mu_out /
 *                       lv_out (nullable); with z (nullable; dtype, row stride ldz): z = mu + eps exp(lv / 2), eps from
 *                       eps_in or (NULL) elements offset .. offset + B L of hlmc_randn's stream `seed`, kept in eps_keep
 *   reparam_bwd_reduce  dz = x w^T (N = L) rounded to dtype; gmu = d_mu + dz, glv = d_lv + dz eps exp(lv / 2) / 2
 *                       (d_mu / d_lv nullable: 0), dtype, row stride ldg
 *   linear_wgrad_pair   hlmc_op_linear_wgrad for two layers reading the same x whose dy are the column halves
 *                       [0, N1) / [N1, 2 N1) of one buffer: one GEMM; ws as for (B = Mb, K, L = N1) */
int64_t hlmc_op_latent_workspace(int dtype, int B, int K, int L);
int hlmc_op_heads_reparam(void* stream, int dtype, const void* x, int ldx, int B, int K, const void* w, int ldw, int L,
                          const float* mu_bias, const float* lv_bias, float* mu, float* lv, float* mu_out, float* lv_out,
                          const float* eps_in, uint64_t seed, uint64_t offset, float* eps_keep, void* z, int ldz,
                          int* S_out, void* ws, int64_t ws_bytes);
int hlmc_op_reparam_bwd_reduce(void* stream, int dtype, const void* x, int ldx, int B, int K, const void* w, int ldw,
                               int L, const float* lv, const float* eps, const float* d_mu, const float* d_lv, void* gmu,
                               void* glv, int ldg, int* S_out, void* ws, int64_t ws_bytes);
int hlmc_op_linear_wgrad_pair(void* stream, int dtype, const void* dy, int lddy, const void* x, int ldx, int Mb, int N1,
                              int K, float* dW1, float* db1, float* dW2, float* db2, void* ws, int64_t ws_bytes);
int64_t hlmc_op_halo_workspace(int Ci, int Co);
int hlmc_op_halo_fwd(void* stream, int kind, const void* x, int B, int Hi, int Wi, int Ci, const void* wp,
                     const float* bias, int Co, void* y, double* out_sums, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                     float* mean_out, float* invstd_out, void* a_out, void* ws, int64_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* HLMC_H_ */
