// The two kernels around the SimpleAutoencoder train step (src/Conditional_VAE.py:252-273, its loop at :428-452) that
// let ONE captured graph serve every step of an epoch:
//   batch_gather  the step's rows of the resident data set into a static [B][d] buffer, the short last batch of an
//                 epoch padded with zero rows, and the row count into device memory (launched outside the graph);
//   mse_rows      mse_loss(reduction="mean") over the first `valid` rows and its gradient, `valid` read from device
//                 memory, so the replayed graph follows it.  The gradient of the padding rows is exactly 0.
// No allocation, no synchronisation, no floating-point atomics: every sum runs in a fixed order.
#include <algorithm>

#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

constexpr int kGatherThreads = 256;
constexpr int kGatherCols = 4 * kGatherThreads;  // columns of one row a block covers
constexpr int kMseThreads = 1024;
constexpr int kMseMaxBlocks = 1024;

inline bool aligned16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// out[b][:] = X[idx[b]][:] for b < count, else 0.  Block (b, c) covers columns [1024 c, 1024 c + 1024) of row b.
// VEC: d % 4 == 0 and both bases 16-byte aligned, so every row is; one float4 per thread.  Otherwise thread t takes the
// columns t, t + 256, t + 512, t + 768 of the block's range (coalesced 4-byte accesses).
// An index outside [0, n) is not dereferenced: the row is written as zeros and *status is set.
template <bool VEC>
__global__ __launch_bounds__(kGatherThreads) void batch_gather_kernel(const float* __restrict__ X, int64_t n, int d,
                                                                      const int64_t* __restrict__ idx, int count,
                                                                      float* __restrict__ out, int* __restrict__ valid_dev,
                                                                      unsigned* status) {
    const int b = blockIdx.x;
    const int t = threadIdx.x;
    if (b == 0 && blockIdx.y == 0 && t == 0) *valid_dev = count;
    const float* src = nullptr;
    if (b < count) {
        const int64_t r = idx[b];
        if (r >= 0 && r < n) src = X + r * (int64_t)d;
        else if (blockIdx.y == 0 && t == 0)
            __hip_atomic_store(status, kDevGatherIndex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    float* dst = out + (int64_t)b * d;
    const int c0 = blockIdx.y * kGatherCols;
    if constexpr (VEC) {
        const int c = c0 + 4 * t;
        if (c < d) {
            const float4 v = src ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(dst + c) = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + t + i * kGatherThreads;
            if (c < d) dst[c] = src ? src[c] : 0.f;
        }
    }
}

// Sum of v over the block in a fixed order: the xor butterfly inside each wave, then wave 0 adds the waves' totals
// (lane l takes wave l's) the same way.  Every thread of the block must call it; thread 0 holds the result.
__device__ double block_sum(double v) {
    __shared__ double wave_tot[kMseThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwaves = (blockDim.x + 63) >> 6;
    __syncthreads();  // a previous call's readers are done with wave_tot
    if (lane == 0) wave_tot[wave] = v;
    __syncthreads();
    if (wave == 0) {
        v = lane < nwaves ? wave_tot[lane] : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    }
    return v;
}

__device__ void mse_finish(double sum, int valid, int d, double* sums2, double* acc) {
    const double cnt = (double)valid * (double)d;
    sums2[0] = sum;
    sums2[1] = cnt;
    if (acc && valid > 0) acc[0] += sum / cnt;
}

// The rows are dense, so element e of the flat [B * d] arrays belongs to a valid row iff e < valid * d.
// g = (float)(((double)r - (double)t) * (2 / (valid d))) there and +0.0f elsewhere (selected, never multiplied: a NaN
// in a padding row of recon reaches neither the gradient nor the sum); the thread adds its squared differences in
// float64 in ascending element order, the block's total goes to part[block] (or, for a one-block grid, straight to
// sums2 / acc).  VEC: d % 4 == 0 and aligned bases: float4 units; a unit never straddles the valid boundary.
template <bool VEC>
__global__ __launch_bounds__(kMseThreads) void mse_rows_kernel(const float* __restrict__ recon,
                                                                const float* __restrict__ target, int B, int d,
                                                                const int* __restrict__ valid_dev,
                                                                float* __restrict__ d_recon, double* __restrict__ part,
                                                                double* sums2, double* acc) {
    const int valid = min(max(*valid_dev, 0), B);
    const int64_t total = (int64_t)B * d, lim = (int64_t)valid * d;
    const double scale = valid > 0 ? 2.0 / ((double)valid * (double)d) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double sum = 0.0;
    if constexpr (VEC) {
        for (int64_t u = first; 4 * u < total; u += stride) {
            const int64_t e = 4 * u;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < lim) {
                const float4 r = *reinterpret_cast<const float4*>(recon + e);
                const float4 t = *reinterpret_cast<const float4*>(target + e);
                const double d0 = (double)r.x - (double)t.x, d1 = (double)r.y - (double)t.y;
                const double d2 = (double)r.z - (double)t.z, d3 = (double)r.w - (double)t.w;
                g = make_float4((float)(d0 * scale), (float)(d1 * scale), (float)(d2 * scale), (float)(d3 * scale));
                sum += d0 * d0;
                sum += d1 * d1;
                sum += d2 * d2;
                sum += d3 * d3;
            }
            *reinterpret_cast<float4*>(d_recon + e) = g;
        }
    } else {
        for (int64_t e = first; e < total; e += stride) {
            float g = 0.f;
            if (e < lim) {
                const double df = (double)recon[e] - (double)target[e];
                g = (float)(df * scale);
                sum += df * df;
            }
            d_recon[e] = g;
        }
    }
    sum = block_sum(sum);
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) mse_finish(sum, valid, d, sums2, acc);
    else part[blockIdx.x] = sum;
}

// the blocks' totals in a fixed order: thread t adds part[t], part[t + 1024], ..., then block_sum
__global__ __launch_bounds__(kMseThreads) void mse_finish_kernel(const double* __restrict__ part, int nparts, int B, int d,
                                                                  const int* __restrict__ valid_dev, double* sums2,
                                                                  double* acc) {
    double sum = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) sum += part[i];
    sum = block_sum(sum);
    if (threadIdx.x == 0) mse_finish(sum, min(max(*valid_dev, 0), B), d, sums2, acc);
}

// blocks of mse_rows_kernel: a function of B * d alone (never of `valid`), non-decreasing in it.  Up to 4096 float4
// units one block does everything in one launch (the autoencoder's 32 x 290 step); above, 2048 units per block.
int mse_blocks(int64_t B, int64_t d) {
    const int64_t units = (B * d + 3) / 4;
    if (units <= 4096) return 1;
    return (int)std::min<int64_t>((units + 2047) / 2048, kMseMaxBlocks);
}

// Step k of an epoch left sums[3 k] = sum (recon - x)^2 and sums[3 k + 2] = sum (1 + lv - mu^2 - exp lv); with its own
// element counts na = na_nl[2 k], nl = na_nl[2 k + 1] (the short last batch differs) the reference's per-step values are
// recon = s0 / na, kl = -0.5 s2 / nl, total = recon + beta kl.  Launched as ONE thread, which adds them in step order,
// each operation rounded once (this file is built without FMA contraction), so a host loop over the same doubles gives
// the same bits.
__global__ void vae_epoch_means_kernel(const double* __restrict__ sums, const int64_t* __restrict__ na_nl, int nb,
                                       double beta, double* __restrict__ out3) {
    double loss = 0.0, recon = 0.0, kl = 0.0;
    for (int k = 0; k < nb; ++k) {
        const double r = sums[3 * k] / (double)na_nl[2 * k];
        const double q = -0.5 * sums[3 * k + 2] / (double)na_nl[2 * k + 1];
        loss += r + beta * q;
        recon += r;
        kl += q;
    }
    out3[0] = loss / (double)nb;
    out3[1] = recon / (double)nb;
    out3[2] = kl / (double)nb;
}

// An epoch of a convolutional VAE fit left one row of loss sums per training step and one per validation batch
// (s[0] = sum (ra - a)^2, s[1] = sum (rt - t)^2, s[2] = sum (1 + lv - mu^2 - exp lv)).  Per row kld = -0.5 s[2] and
// total = (s[0] + text_weight s[1]) + beta kld, in that association.  ONE thread adds the rows in step order, each
// operation rounded once (no FMA contraction in this file), so a host loop over the same doubles gives the same bits.
__global__ void fit_epoch_totals_kernel(const double* __restrict__ train_sums, int nt,
                                        const double* __restrict__ val_sums, int nv, double text_weight, double beta,
                                        double train_div, double val_div, double* __restrict__ out5) {
    double total = 0.0, audio = 0.0, text = 0.0, kld = 0.0, val = 0.0;
    for (int k = 0; k < nt; ++k) {
        const double* s = train_sums + 3 * k;
        const double q = -0.5 * s[2];
        const double tw = text_weight * s[1];
        const double bq = beta * q;
        total += (s[0] + tw) + bq;
        audio += s[0];
        text += s[1];
        kld += q;
    }
    for (int k = 0; k < nv; ++k) {
        const double* s = val_sums + 3 * k;
        const double q = -0.5 * s[2];
        const double tw = text_weight * s[1];
        const double bq = beta * q;
        val += (s[0] + tw) + bq;
    }
    out5[0] = total / train_div;
    out5[1] = audio / train_div;
    out5[2] = text / train_div;
    out5[3] = kld / train_div;
    out5[4] = val / val_div;
}

}  // namespace

namespace ae {

int fit_epoch_totals(hipStream_t s, const double* train_sums, int nt, const double* val_sums, int nv,
                     double text_weight, double beta, double train_div, double val_div, double* out5) {
    HLMC_CHECK_ARG(train_sums && val_sums && out5, "fit_epoch_totals: NULL argument");
    HLMC_CHECK_ARG(nt >= 1 && nv >= 1, "fit_epoch_totals: need nt >= 1 and nv >= 1");
    HLMC_CHECK_ARG(text_weight == text_weight && beta == beta, "fit_epoch_totals: text_weight or beta is NaN");
    HLMC_CHECK_ARG(train_div > 0.0 && val_div > 0.0, "fit_epoch_totals: need train_div > 0 and val_div > 0");
    fit_epoch_totals_kernel<<<1, 1, 0, s>>>(train_sums, nt, val_sums, nv, text_weight, beta, train_div, val_div, out5);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int vae_epoch_means(hipStream_t s, const double* sums, const int64_t* na_nl, int nb, double beta, double* out3) {
    HLMC_CHECK_ARG(sums && na_nl && out3, "vae_epoch_means: NULL argument");
    HLMC_CHECK_ARG(nb >= 1, "vae_epoch_means: need nb >= 1");
    HLMC_CHECK_ARG(beta == beta, "vae_epoch_means: beta is NaN");
    vae_epoch_means_kernel<<<1, 1, 0, s>>>(sums, na_nl, nb, beta, out3);
    HLMC_LAUNCHED();
    return HLMC_OK;
}


int batch_gather(hipStream_t s, const float* X, int64_t n, int d, const int64_t* idx, int count, int B, float* out,
                 int* valid_dev) {
    HLMC_CHECK_ARG(X && idx && out && valid_dev, "batch_gather: NULL argument");
    HLMC_CHECK_ARG(n >= 1 && d >= 1, "batch_gather: need n >= 1 and d >= 1");
    HLMC_CHECK_ARG(B >= 1, "batch_gather: need B >= 1");
    HLMC_CHECK_ARG(count >= 1 && count <= B, "batch_gather: need 1 <= count <= B");
    unsigned* status = ops::dev_status_word();
    HLMC_CHECK_ARG(status, "batch_gather: no device status word (hipHostMalloc failed)");
    const dim3 grid((unsigned)B, (unsigned)((d + kGatherCols - 1) / kGatherCols));
    HLMC_CHECK_ARG(grid.y <= 65535, "batch_gather: d too large");
    const bool vec = d % 4 == 0 && aligned16p(X) && aligned16p(out);
    if (vec)
        batch_gather_kernel<true><<<grid, kGatherThreads, 0, s>>>(X, n, d, idx, count, out, valid_dev, status + 1);
    else
        batch_gather_kernel<false><<<grid, kGatherThreads, 0, s>>>(X, n, d, idx, count, out, valid_dev, status + 1);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

size_t mse_rows_workspace(int64_t B, int64_t d) {
    if (B < 1 || d < 1 || B > INT32_MAX || d > INT32_MAX) return 0;
    return align256((size_t)mse_blocks(B, d) * sizeof(double));
}

int mse_rows(hipStream_t s, const float* recon, const float* target, int B, int d, const int* valid_dev, float* d_recon,
             double* sums2, double* acc, void* ws) {
    HLMC_CHECK_ARG(recon && target && valid_dev && d_recon && sums2 && ws, "mse_rows: NULL argument");
    HLMC_CHECK_ARG(B >= 1 && d >= 1, "mse_rows: need B >= 1 and d >= 1");
    const int G = mse_blocks(B, d);
    double* part = static_cast<double*>(ws);
    const bool vec = d % 4 == 0 && aligned16p(recon) && aligned16p(target) && aligned16p(d_recon);
    if (vec)
        mse_rows_kernel<true><<<G, kMseThreads, 0, s>>>(recon, target, B, d, valid_dev, d_recon, part, sums2, acc);
    else
        mse_rows_kernel<false><<<G, kMseThreads, 0, s>>>(recon, target, B, d, valid_dev, d_recon, part, sums2, acc);
    HLMC_LAUNCHED();
    if (G > 1) {
        mse_finish_kernel<<<1, kMseThreads, 0, s>>>(part, G, B, d, valid_dev, sums2, acc);
        HLMC_LAUNCHED();
    }
    return HLMC_OK;
}

}  // namespace ae
}  // namespace hlmc
