// PCA on the GPU (sklearn.decomposition.PCA at src/Simple_VAE.py:258-263 and src/Conditional_VAE.py:422-425): the two
// heavy steps of the exact decomposition, both float64 GEMMs on v_mfma_f64_16x16x4_f64 over float32 data.
//
// cov: the column mean and the centred Gram matrix G = (X - m)^T (X - m), two passes over X.
//   Pass 1: float64 column sums per row slab (4 row groups per block, each in row order, combined 0..3), the slabs
//   summed in slab order, mean = sum / n.
//   Pass 2: one block per (upper-triangle 64 x 64 feature-tile pair, row slab) on the tile of f64tile.hpp, the sample
//   index as K and both operands k-major images (X's rows are the inner axis), centred in float64 when they are
//   stored ((double)x - mean; a row past the slab's end is 0, not -mean).  The slab's partial tile goes to the
//   workspace; a second kernel sums the slabs in slab order and writes G[i][j] and G[j][i] from the same value (of a
//   diagonal tile only the entries i <= j are used), so G is symmetric bit for bit.
//   The slab length depends on n alone, no float atomics: the result is bit-identical from run to run.
//
// project: out = (A - a_off) B + o_off, A float32 [n][p] (row image), B float64 [p][q] (k-major image), accumulated
//   in float64 on the MFMA and rounded once to float32.  transform, inverse_transform and whitening are this one
//   kernel with different B and offsets.
//
// Rounding count, assuming the MFMA's 4-step inner sum rounds each product and each addition at most
// once: a Gram entry takes one rounding per centred factor, one per product and n - 1 additions of nonzero terms (the
// zero fill adds exact zeros), (n + 2) 2^-53 sum |xc_i xc_j| in all; a projection entry p + 2 roundings.
#include <algorithm>
#include <cstdint>

#include "f64tile.hpp"
#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

using namespace f64tile;   // kTile: features (cov) / rows and columns (project); kKC: sample rows / inner columns

constexpr int kSlabMin = 256;    // shortest row slab
constexpr int kSlabsMax = 128;   // most row slabs (bounds the workspace at 128 partial Gram matrices)
constexpr int64_t kMaxN = (int64_t)1 << 24;
constexpr int kMaxD = 1024;

// rows per slab: a function of n alone
int64_t slab_len(int64_t n) {
    const int64_t per = (n + kSlabsMax - 1) / kSlabsMax;
    return std::max<int64_t>(kSlabMin, (per + 31) / 32 * 32);
}

struct Layout {
    int64_t slab, slabs;
    int tiles, pairs;
    size_t colsum, part, total;
};

Layout layout(int64_t n, int d) {
    Layout l;
    l.slab = slab_len(n);
    l.slabs = (n + l.slab - 1) / l.slab;
    l.tiles = (d + kTile - 1) / kTile;
    l.pairs = l.tiles * (l.tiles + 1) / 2;
    Carver c;
    l.colsum = c.take((size_t)l.slabs * (size_t)d * sizeof(double));
    l.part = c.take((size_t)l.slabs * (size_t)l.pairs * kTile * kTile * sizeof(double));
    l.total = c.off;
    return l;
}

// colsum[slab][c] = sum of the slab's rows of column c in float64: 64 columns x 4 row groups per block, a group
// adds its rows r0 + g, r0 + g + 4, ... in that order, the groups are combined 0, 1, 2, 3
__global__ __launch_bounds__(256) void pca_colsum_kernel(const float* __restrict__ X, int64_t n, int d, int64_t slab,
                                                         double* __restrict__ colsum) {
    __shared__ double part[4][kTile];
    const int c = blockIdx.x * kTile + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = min(n, r0 + slab);
    double s = 0.0;
    if (c < d)
        for (int64_t r = r0 + g; r < r1; r += 4) s += (double)X[r * d + c];
    part[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < d)
        colsum[(size_t)blockIdx.y * d + c] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) +
                                             part[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void pca_mean_kernel(const double* __restrict__ colsum, int64_t n, int d,
                                                       int64_t slabs, double* __restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int64_t b = 0; b < slabs; ++b) s += colsum[(size_t)b * d + c];
    mean[c] = s / (double)n;
}

// upper-triangle pair index (row-major: (0,0) (0,1) .. (0,T-1) (1,1) ..) -> feature tiles ti <= tj
__device__ __forceinline__ void pair_tiles(int pair, int tiles, int& ti, int& tj) {
    ti = 0;
    while (pair >= tiles - ti) {
        pair -= tiles - ti;
        ++ti;
    }
    tj = ti + pair;
}

// part[slab][pair][64][64] = sum over the slab's rows of xc[r][64 ti + i] xc[r][64 tj + j].  4 waves, wave w owns
// features 16 w .. 16 w + 15 of tile ti against the 64 features of tile tj (4 MFMA tiles).
__global__ __launch_bounds__(256) void pca_gram_kernel(const float* __restrict__ X, const double* __restrict__ mean,
                                                       int64_t n, int d, int64_t slab, int tiles, int pairs,
                                                       double* __restrict__ part) {
    __shared__ double a_sh[KImage::kDoubles];
    __shared__ double b_sh[KImage::kDoubles];
    int ti, tj;
    pair_tiles(blockIdx.x, tiles, ti, tj);
    const bool diag = ti == tj;   // one image serves both operands: the second is neither fetched nor stored
    const KImage As{a_sh}, Bs{diag ? a_sh : b_sh};
    const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = min(n, r0 + slab);
    Stage<KImage, float> pa, pb;   // the next chunk is fetched into registers while the MFMAs of this one run
    // the column of each tile that the thread stages, and its mean
    const int ci = ti * kTile + pa.minor(), cj = tj * kTile + pb.minor();
    const double mi = ci < d ? mean[ci] : 0.0, mj = cj < d ? mean[cj] : 0.0;
    double4_t acc[4] = {};
    pa.fetch(X, d, r0, r1, ti * kTile, d);
    if (!diag) pb.fetch(X, d, r0, r1, tj * kTile, d);
    for (int64_t k0 = r0; k0 < r1; k0 += kKC) {
        __syncthreads();
        // centred where it is stored; a row past the slab contributes 0, not -mean
        pa.commit(As, [mi](double x) { return x - mi; });
        if (!diag) pb.commit(Bs, [mj](double x) { return x - mj; });
        __syncthreads();
        if (k0 + kKC < r1) {
            pa.fetch(X, d, k0 + kKC, r1, ti * kTile, d);
            if (!diag) pb.fetch(X, d, k0 + kKC, r1, tj * kTile, d);
        }
        mma_chunk(acc, As, Bs, k_steps(r1 - k0));
    }
    double* out = part + ((size_t)blockIdx.y * pairs + blockIdx.x) * (kTile * kTile);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) out[acc_row(q) * kTile + acc_col(t)] = acc[t][q];
}

// G[i][j] = G[j][i] = sum over the slabs, in slab order, of the pair's partial tiles; one block per pair
__global__ __launch_bounds__(256) void pca_gram_sum_kernel(const double* __restrict__ part, int d, int64_t slabs,
                                                           int tiles, int pairs, double* __restrict__ G) {
    int ti, tj;
    pair_tiles(blockIdx.x, tiles, ti, tj);
    for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
        const int r = e / kTile, c = e - r * kTile;
        const int i = ti * kTile + r, j = tj * kTile + c;
        if (i >= d || j >= d || (ti == tj && r > c)) continue;
        double s = 0.0;
        for (int64_t b = 0; b < slabs; ++b) s += part[((size_t)b * pairs + blockIdx.x) * (kTile * kTile) + e];
        G[(size_t)i * d + j] = s;
        G[(size_t)j * d + i] = s;
    }
}

// out[r][j] = (float)(sum_c ((double)A[r][c] - a_off[c]) B[c][j] + o_off[j]); one 64 x 64 tile per block, wave w
// owns rows 16 w .. 16 w + 15
__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ A, int64_t n, int p,
                                                          const double* __restrict__ B, int q,
                                                          const double* __restrict__ a_off,
                                                          const double* __restrict__ o_off, float* __restrict__ out) {
    __shared__ double a_sh[RowImage::kDoubles];
    __shared__ double b_sh[KImage::kDoubles];
    const RowImage As{a_sh};
    const KImage Bs{b_sh};
    const int64_t i0 = (int64_t)blockIdx.x * kTile;
    const int j0 = blockIdx.y * kTile;
    double4_t acc[4] = {};
    // the next chunk, and a_off of the thread's inner column of A, is fetched while the MFMAs of this one run
    Stage<RowImage, float> pa;
    Stage<KImage, double> pb;
    double off;
    auto fetch = [&](int k0) {
        const int c = k0 + pa.minor();
        off = (c < p && a_off) ? a_off[c] : 0.0;
        pa.fetch(A, p, i0, n, k0, p);
        pb.fetch(B, q, k0, p, j0, q);
    };
    fetch(0);
    for (int k0 = 0; k0 < p; k0 += kKC) {
        __syncthreads();
        pa.commit(As, [off](double x) { return x - off; });
        pb.commit(Bs);
        __syncthreads();
        if (k0 + kKC < p) fetch(k0 + kKC);
        mma_chunk(acc, As, Bs, k_steps(p - k0));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = j0 + acc_col(t);
        if (j >= q) continue;
        const double oo = o_off ? o_off[j] : 0.0;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int64_t r = i0 + acc_row(qq);
            if (r < n) out[r * q + j] = (float)(acc[t][qq] + oo);
        }
    }
}

}  // namespace

namespace pca {

size_t workspace(int64_t n, int d) {
    if (n < 2 || n > kMaxN || d < 1 || d > kMaxD) return 0;
    return layout(n, d).total;
}

int cov(hipStream_t s, const float* X, int64_t n, int d, double* mean, double* G, void* ws, size_t ws_bytes) {
    HLMC_CHECK_ARG(X && mean && G && ws, "pca_cov: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "pca_cov: need 2 <= n <= 16777216");
    HLMC_CHECK_ARG(d >= 1 && d <= kMaxD, "pca_cov: need 1 <= d <= 1024");
    const Layout l = layout(n, d);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "pca_cov: workspace too small (hlmc_pca_workspace)");
    char* w = static_cast<char*>(ws);
    double* colsum = reinterpret_cast<double*>(w + l.colsum);
    double* part = reinterpret_cast<double*>(w + l.part);
    pca_colsum_kernel<<<dim3((unsigned)l.tiles, (unsigned)l.slabs), 256, 0, s>>>(X, n, d, l.slab, colsum);
    HLMC_LAUNCHED();
    pca_mean_kernel<<<(unsigned)((d + 255) / 256), 256, 0, s>>>(colsum, n, d, l.slabs, mean);
    HLMC_LAUNCHED();
    pca_gram_kernel<<<dim3((unsigned)l.pairs, (unsigned)l.slabs), 256, 0, s>>>(X, mean, n, d, l.slab, l.tiles, l.pairs,
                                                                              part);
    HLMC_LAUNCHED();
    pca_gram_sum_kernel<<<(unsigned)l.pairs, 256, 0, s>>>(part, d, l.slabs, l.tiles, l.pairs, G);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int project(hipStream_t s, const float* A, int64_t n, int p, const double* B, int q, const double* a_off,
            const double* o_off, float* out) {
    HLMC_CHECK_ARG(A && B && out, "pca_project: NULL argument");
    HLMC_CHECK_ARG(n >= 1 && n <= INT32_MAX, "pca_project: need 1 <= n < 2^31");
    HLMC_CHECK_ARG(p >= 1 && p <= kMaxD, "pca_project: need 1 <= p <= 1024");
    HLMC_CHECK_ARG(q >= 1 && q <= kMaxD, "pca_project: need 1 <= q <= 1024");
    const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)((q + kTile - 1) / kTile));
    pca_project_kernel<<<grid, 256, 0, s>>>(A, n, p, B, q, a_off, o_off, out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

}  // namespace pca
}  // namespace hlmc
