// Ward agglomerative clustering on the GPU with sklearn's tree (sklearn.cluster.AgglomerativeClustering(n_clusters=k)
// at src/Convolutional_VAE.py:334-342,381 = scipy.cluster.hierarchy.ward on the float64-upcast rows).
//
// ward_pdist_kernel: the full symmetric n x n float64 distance matrix.  Per pair s = 0, then for k = 0 .. d-1 in
// that order t = a_k - b_k, s = s + t * t (this file is built with -ffp-contract=off: no FMA), D = sqrt(s): the
// arithmetic of scipy's pdist, so the MFMA form |a|^2 + |b|^2 - 2 a.b (another rounding) is not an option.
// (a - b)^2 = (b - a)^2 exactly, so only the upper-triangle tiles are computed and each is stored twice.
//
// ward_chain_kernel: the nearest-neighbour chain, n - 1 merges with the Lance-Williams Ward update, in one launch
// of ONE workgroup.  The algorithm is sequential across merges and parallel only inside a step (a row scan, a row
// update), so a single workgroup needs nothing but __syncthreads: no grid-wide synchronisation, no spin-wait, no
// arrival counter.  Every loop is bounded by n; a scan that finds no neighbour (NaN in D) or an exhausted bound
// ends the kernel with a non-zero status word.
#include <climits>

#include "f64tile.hpp"
#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

using f64tile::kKC;
using f64tile::kTile;
using f64tile::RowImage;
constexpr int kTS = kTile + 1;   // stride of the transposed-store staging tile (130 dwords = 2 mod 64)
constexpr int64_t kMaxN = 32768; // D is 8 GiB at the cap; size[] fills 128 KB of LDS
constexpr int kChainThreads = 1024;
constexpr int kWaves = kChainThreads / 64;

constexpr int kStatusNoNeighbour = 1;   // a scan found nothing smaller than +inf: NaN (or +inf) in D
constexpr int kStatusBound = 2;         // chain longer than n or more than 4 n scans

// One 64 x 64 tile of distances per block (256 threads, a 4 x 4 register block each: rows ty + 16 q, columns
// tx + 16 t) from the two row images of f64tile.hpp, read here by plain loads.  Blocks below the diagonal return at
// once.
__global__ __launch_bounds__(256) void ward_pdist_kernel(const float* __restrict__ X, int64_t n, int d,
                                                         double* __restrict__ D) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double sh[2 * RowImage::kDoubles];   // As | Bs, reused as the [64][kTS] staging tile (4160 <= 4352)
    const RowImage As{sh}, Bs{sh + RowImage::kDoubles};
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.y * kTile, j0 = (int64_t)blockIdx.x * kTile;
    double s[4][4] = {};
    // the next K chunk is fetched into registers while this one is summed; the rows past n are zero-filled and never
    // stored
    f64tile::Stage<RowImage, float> pa, pb;
    pa.fetch(X, d, i0, n, 0, d);
    pb.fetch(X, d, j0, n, 0, d);
    for (int k0 = 0; k0 < d; k0 += kKC) {
        __syncthreads();
        pa.commit(As);
        pb.commit(Bs);
        __syncthreads();
        if (k0 + kKC < d) {
            pa.fetch(X, d, i0, n, k0 + kKC, d);
            pb.fetch(X, d, j0, n, k0 + kKC, d);
        }
        const int kmax = min(kKC, d - k0);
        for (int kk = 0; kk < kmax; ++kk) {   // sequential in k: the order of the sum is part of the result
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = As.el(ty + 16 * q, kk);
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = Bs.el(tx + 16 * t, kk);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double df = a[q] - b[t];
                    s[q][t] = s[q][t] + df * df;
                }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) s[q][t] = sqrt(s[q][t]);
    // D[i][j]: 16 consecutive columns per half-wave row
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t gi = i0 + ty + 16 * q;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t gj = j0 + tx + 16 * t;
            if (gi < n && gj < n) D[gi * n + gj] = s[q][t];
        }
    }
    if (blockIdx.x == blockIdx.y) return;   // a diagonal tile holds both halves already (and 0 on the diagonal)
    // D[j][i]: transpose through LDS so that these stores run along rows as well
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) sh[(ty + 16 * q) * kTS + tx + 16 * t] = s[q][t];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t gj = j0 + ty + 16 * q;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t gi = i0 + tx + 16 * t;
            if (gi < n && gj < n) D[gj * n + gi] = sh[(tx + 16 * t) * kTS + ty + 16 * q];
        }
    }
}

// Lance-Williams for Ward, scipy's expression evaluated left to right (no FMA: -ffp-contract=off)
__device__ __forceinline__ double ward_update(double dxi, double dyi, double dxy, int nx, int ny, int ni) {
    const double t = 1.0 / (double)(ni + nx + ny);
    const double a = (((double)(ni + nx) * t) * dxi) * dxi;
    const double b = (((double)(ni + ny) * t) * dyi) * dyi;
    const double c = (((double)ni * t) * dxy) * dxy;
    return sqrt((a + b) - c);
}

// The whole chain in one workgroup.  x (chain top), y0 (its predecessor or -1), len (chain length) and lo (no live
// index lies below it) are held by every thread and stay uniform: each thread computes them from the same LDS words.
// chain[] is written by thread 0 only, at least one barrier before anything reads the entry.
__global__ __launch_bounds__(kChainThreads) void ward_chain_kernel(int n, double* D, int32_t* chain,
                                                                   int32_t* __restrict__ merge_a,
                                                                   int32_t* __restrict__ merge_b,
                                                                   double* __restrict__ merge_dist,
                                                                   int32_t* __restrict__ merge_size,
                                                                   int32_t* __restrict__ status) {
    extern __shared__ int32_t size[];            // [n] points per live cluster, 0 = merged away
    __shared__ double red_v[2][kWaves];          // per-wave scan minima, double-buffered: one barrier per scan
    __shared__ int red_i[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t ns = (size_t)n;
    for (int i = tid; i < n; i += kChainThreads) size[i] = 1;
    __syncthreads();

    const int max_scans = 4 * n;   // pushes <= 2 (n - 1) pops + n left over; a scan pushes or merges: < 4 n scans
    int merges = 0, len = 0, lo = 0, x = -1, y0 = -1, par = 0, fail = 0;
    for (int scan = 0; scan < max_scans && merges < n - 1; ++scan) {
        if (len == 0) {   // chain start: the lowest live index (clusters never come back, so lo only grows)
            while (lo < n && size[lo] == 0) ++lo;
            if (lo >= n) { fail = kStatusBound; break; }
            x = lo;
            y0 = -1;
            len = 1;
            if (tid == 0) chain[0] = x;
        }
        const double* row = D + (size_t)x * ns;
        const double cur0 = y0 >= 0 ? row[y0] : __builtin_inf();
        // block argmin of row x over the live i != x; ties go to the lowest index (strict <, ascending i)
        double best = __builtin_inf();
        int bi = INT_MAX;
        for (int i = tid; i < n; i += kChainThreads) {
            if (size[i] == 0 || i == x) continue;
            const double v = row[i];
            if (v < best) { best = v; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { red_v[par][wv] = best; red_i[par][wv] = bi; }
        __syncthreads();
        best = red_v[par][0];
        bi = red_i[par][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            const double ov = red_v[par][w];
            const int oi = red_i[par][w];
            if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        par ^= 1;
        // the predecessor is kept unless something is strictly closer
        int y = y0;
        double cur = cur0;
        if (best < cur0) { y = bi; cur = best; }
        if (y < 0 || y >= n) { fail = kStatusNoNeighbour; break; }
        if (y != y0) {   // push
            if (len >= n) { fail = kStatusBound; break; }
            if (tid == 0) chain[len] = y;
            ++len;
            y0 = x;
            x = y;
            continue;
        }
        // reciprocal nearest neighbours: merge a < b, a dies, b carries the cluster
        const int a = x < y ? x : y, b = x < y ? y : x;
        const int na = size[a], nb = size[b];
        const double* ra = D + (size_t)a * ns;
        double* rb = D + (size_t)b * ns;
        for (int i = tid; i < n; i += kChainThreads) {
            const int ni = size[i];
            if (ni == 0 || i == a || i == b) continue;
            const double v = ward_update(ra[i], rb[i], cur, na, nb, ni);
            rb[i] = v;
            D[(size_t)i * ns + (size_t)b] = v;
        }
        __syncthreads();   // every thread has read size[a], size[b]; the new distances are written
        if (tid == 0) {
            merge_a[merges] = a;
            merge_b[merges] = b;
            merge_dist[merges] = cur;
            merge_size[merges] = na + nb;
            size[a] = 0;
            size[b] = na + nb;
        }
        __syncthreads();
        ++merges;
        len -= 2;
        if (len > 0) {   // entries written by thread 0 at least two barriers ago
            x = __hip_atomic_load(chain + len - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            y0 = len > 1 ? __hip_atomic_load(chain + len - 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : -1;
            if (x < 0 || x >= n || y0 >= n) { fail = kStatusBound; break; }
        }
    }
    if (fail == 0 && merges < n - 1) fail = kStatusBound;
    if (tid == 0) status[0] = fail;
}

struct Layout {
    size_t D, status, chain, total;
};

Layout layout(int64_t n) {
    Carver c;
    Layout l;
    l.D = c.take((size_t)n * (size_t)n * sizeof(double));   // first: callers pass the workspace itself as D
    l.status = c.take(sizeof(int32_t));
    l.chain = c.take((size_t)n * sizeof(int32_t));
    l.total = c.off;
    return l;
}

}  // namespace

namespace ward {

size_t workspace(int64_t n) {
    if (n < 2 || n > kMaxN) return 0;
    return layout(n).total;
}

int pdist(hipStream_t s, const float* X, int64_t n, int d, double* D) {
    HLMC_CHECK_ARG(X && D, "ward_pdist: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN && d >= 1, "ward_pdist: need 2 <= n <= 32768 and d >= 1");
    const unsigned T = (unsigned)((n + kTile - 1) / kTile);
    ward_pdist_kernel<<<dim3(T, T), 256, 0, s>>>(X, n, d, D);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int chain(hipStream_t s, int64_t n, double* D, int32_t* merge_a, int32_t* merge_b, double* merge_dist,
          int32_t* merge_size, void* ws, size_t ws_bytes) {
    HLMC_CHECK_ARG(D && merge_a && merge_b && merge_dist && merge_size && ws, "ward_chain: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "ward_chain: need 2 <= n <= 32768");
    const Layout l = layout(n);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "ward_chain: workspace too small (hlmc_ward_workspace)");
    char* w = static_cast<char*>(ws);
    int32_t* status = reinterpret_cast<int32_t*>(w + l.status);
    int32_t* chain_buf = reinterpret_cast<int32_t*>(w + l.chain);
    // the kernel overwrites the word at its end: a launch that never finished reads back as non-zero too
    HLMC_HIP(hipMemsetAsync(status, 0xff, sizeof(int32_t), s));
    ward_chain_kernel<<<1, kChainThreads, (size_t)n * sizeof(int32_t), s>>>((int)n, D, chain_buf, merge_a, merge_b,
                                                                            merge_dist, merge_size, status);
    HLMC_LAUNCHED();
    int32_t st = -1;
    HLMC_HIP(hipMemcpyAsync(&st, status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HLMC_HIP(hipStreamSynchronize(s));
    if (st != 0) {
        set_error("ward_chain: device status " + std::to_string(st) +
                  (st == kStatusNoNeighbour ? " (a scan found no neighbour: NaN or infinite distance)"
                                            : " (a loop bound computed from n was exhausted)"));
        return HLMC_EDEVICE;
    }
    return HLMC_OK;
}

}  // namespace ward
}  // namespace hlmc
