// DBSCAN on the GPU with sklearn's labels (sklearn.cluster.DBSCAN(eps, min_samples).fit_predict at
// src/Convolutional_VAE.py:353-354,382; brute-force float32 path of sklearn 1.7).
//
// Neighbourhood pass (one pass over the distance tiles serves all E radii of a sweep):
//   i ~ j  iff  max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) <= r_e        (everything float64 on the upcast float32 rows)
// x_i.x_j comes from the fp64 MFMA tile of f64tile.hpp (both operands row images); a tile is 64 columns wide so one
// tile row is one word of the bit-packed adjacency adj[e][i][j / 64].  The expression
// (n_i + n_j) - 2 dot is symmetric in i and j bit for bit (the MFMA sums over k in the same order for (i, j) and
// (j, i)), so the adjacency is symmetric.  A pair within 4 (d + 4) 2^-53 (n_i + n_j) of a threshold is counted as
// borderline (another summation order could flip it); the count is reported, nothing else changes.
//
// Labelling pass (per radius, on the bits alone): core flags -> lock-free union-find over core-core bits, the
// larger root always hooked under the smaller (so a component's root is its smallest core index, whatever the
// order of the races) -> flatten -> number the roots by a prefix sum in index order (sklearn numbers clusters in
// increasing order of their first core point) -> a border point takes the smallest cluster number among its
// core neighbours (dbscan_inner reaches it first from the lowest-numbered cluster) -> noise is -1.
// Integer atomics only; every output is the unique fixed point, identical from run to run.
#include <algorithm>
#include <climits>

#include "f64tile.hpp"
#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

using namespace f64tile;
typedef unsigned long long u64;

constexpr int kMaxRadii = 32;    // radii per launch (kernel argument block)

struct Radii {
    double r[kMaxRadii];
};

// float64 squared row norms of the float32 rows: one wave per row, fixed order
__global__ __launch_bounds__(256) void db_norms_kernel(const float* __restrict__ X, int64_t n, int d,
                                                       double* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double s = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double v = (double)X[i * d + c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) norms[i] = s;
}

// One 64 x 64 tile of squared distances per block (4 waves, 16 rows x 64 columns each = 4 MFMA tiles), compared
// against every radius: adj[e][i][blockIdx.x] for the block's rows, and the borderline pairs (i < j) per radius.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void db_neigh_kernel(const float* __restrict__ X, const double* __restrict__ norms,
                                                       int64_t n, int d, Radii R, int E, double tolc,
                                                       u64* __restrict__ adj, int64_t W, u64* __restrict__ border) {
    __shared__ double a_sh[RowImage::kDoubles];
    __shared__ double b_sh[RowImage::kDoubles];
    const RowImage As{a_sh}, Bs{b_sh};
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.y * kTile, j0 = (int64_t)blockIdx.x * kTile;
    double4_t acc[4] = {};
    Stage<RowImage, float> pa, pb;   // the next K chunk is fetched into registers while the MFMAs of this one run
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
        mma_chunk(acc, As, Bs, k_steps(d - k0));
    }
    double d2[4][4], tol[4][4];
    bool valid[4][4], upper[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t gi = i0 + acc_row(q);
        const double ni = gi < n ? norms[gi] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t gj = j0 + acc_col(t);
            const double nj = gj < n ? norms[gj] : 0.0;
            const double sn = ni + nj;
            d2[t][q] = fmax(0.0, sn - 2.0 * acc[t][q]);
            tol[t][q] = tolc * sn;
            valid[t][q] = gi < n && gj < n;
            upper[t][q] = valid[t][q] && gi < gj;
        }
    }
    for (int e = 0; e < E; ++e) {
        const double r = R.r[e];
        int nb = 0;
        u64* arow = adj + (size_t)e * (size_t)n * (size_t)W;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u64 word = 0;   // lanes 0..3: the word of row wv * 16 + 4 q + lane
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double diff = d2[t][q] - r;
                const u64 b = __ballot(valid[t][q] && d2[t][q] <= r);
                // ballot bits [16 g, 16 g + 16) are row g + 4 q, columns 16 t .. 16 t + 15 (acc_row, acc_col)
                word |= ((b >> (16 * (lane & 3))) & 0xffffull) << (16 * t);
                nb += (upper[t][q] && fabs(diff) <= tol[t][q]) ? 1 : 0;
            }
            const int64_t gi = i0 + wv * 16 + 4 * q + lane;
            if (lane < 4 && gi < n) arow[(size_t)gi * (size_t)W + blockIdx.x] = word;
        }
        if (__ballot(nb > 0)) {   // rare: integer atomic, order-independent
            const int tot = wave_sum(nb);
            if (lane == 0) atomicAdd(&border[e], (u64)tot);
        }
    }
}

// counts[e][i] = popcount of row i of adj[e]: one wave per row
__global__ __launch_bounds__(256) void db_count_kernel(const u64* __restrict__ adj, int64_t n, int64_t W, int E,
                                                       int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // over E * n
    if (row >= (int64_t)E * n) return;
    const u64* a = adj + (size_t)row * (size_t)W;
    int c = 0;
    for (int64_t w = lane; w < W; w += 64) c += __popcll(a[w]);
    c = wave_sum(c);
    if (lane == 0) counts[row] = c;
}

// ---------------------------------------------------------------------------------------------- labelling
__device__ __forceinline__ int ld_rel(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_rel(int32_t* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x with path halving.  parent[] only ever points to a smaller index (an ancestor), a non-root never
// becomes a root again, and only roots are hooked (by compare-and-swap), so the racing plain stores are safe.
__device__ int uf_find(int32_t* parent, int x) {
    for (;;) {
        const int r = ld_rel(parent + x);
        if (r == x) return x;
        const int g = ld_rel(parent + r);
        if (g != r) st_rel(parent + x, g);
        x = g;
    }
}

__device__ void uf_unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // hook the larger root under the smaller
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

// core flags, the core bit mask, parent[i] = i.  Grid covers 64 * W threads so every mask word is written.
__global__ __launch_bounds__(256) void db_core_kernel(const int32_t* __restrict__ counts, int64_t n, int min_samples,
                                                      uint8_t* __restrict__ core, u64* __restrict__ corebits,
                                                      int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool c = i < n && counts[i] >= min_samples;
    const u64 b = __ballot(c);
    if (i < n) {
        core[i] = c ? 1 : 0;
        parent[i] = (int32_t)i;
    }
    if ((threadIdx.x & 63) == 0 && i < n) corebits[i >> 6] = b;
}

// one wave per core row i: unite i with every core neighbour j < i (the adjacency is symmetric)
__global__ __launch_bounds__(256) void db_union_kernel(const u64* __restrict__ adj, int64_t n, int64_t W,
                                                       const uint8_t* __restrict__ core,
                                                       const u64* __restrict__ corebits, int32_t* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n || !core[i]) return;
    const u64* a = adj + (size_t)i * (size_t)W;
    const int64_t wl = i >> 6;
    for (int64_t w = lane; w <= wl; w += 64) {
        u64 m = a[w] & corebits[w];
        if (w == wl) m &= (1ull << (i & 63)) - 1ull;
        while (m) {
            const int j = (int)(w * 64 + __builtin_ctzll(m));
            m &= m - 1;
            uf_unite(parent, (int)i, j);
        }
    }
}

// root[i] = the component's smallest core index (read-only walk: all unions are complete), -1 for non-core
__global__ __launch_bounds__(256) void db_flatten_kernel(const int32_t* __restrict__ parent, int64_t n,
                                                         const uint8_t* __restrict__ core, int32_t* __restrict__ root) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x = -1;
    if (core[i]) {
        x = (int)i;
        for (int p = parent[x]; p != x; p = parent[x]) x = p;
    }
    root[i] = x;
}

// cid[i] for the roots = number of roots before i (exclusive prefix sum in index order); one block
__global__ __launch_bounds__(1024) void db_number_kernel(const int32_t* __restrict__ root, int64_t n,
                                                         int32_t* __restrict__ cid, int32_t* __restrict__ n_clusters) {
    __shared__ int sums[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
    int c = 0;
    for (int64_t i = b; i < e; ++i) c += root[i] == (int32_t)i ? 1 : 0;
    sums[tid] = c;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // inclusive scan of the per-thread sums
        const int v = tid >= o ? sums[tid - o] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int base = sums[tid] - c;
    for (int64_t i = b; i < e; ++i)
        if (root[i] == (int32_t)i) cid[i] = base++;
    if (tid == 1023 && n_clusters) n_clusters[0] = sums[1023];
}

// one wave per row: a core point takes its root's number, a border point the smallest number among its core
// neighbours (= the smallest root, numbers grow with the root index), anything else -1
__global__ __launch_bounds__(256) void db_label_kernel(const u64* __restrict__ adj, int64_t n, int64_t W,
                                                       const uint8_t* __restrict__ core,
                                                       const u64* __restrict__ corebits,
                                                       const int32_t* __restrict__ root, const int32_t* __restrict__ cid,
                                                       int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    if (core[i]) {
        if (lane == 0) labels[i] = cid[root[i]];
        return;
    }
    const u64* a = adj + (size_t)i * (size_t)W;
    int best = INT_MAX;
    for (int64_t w = lane; w < W; w += 64) {
        u64 m = a[w] & corebits[w];
        while (m) {
            const int j = (int)(w * 64 + __builtin_ctzll(m));
            m &= m - 1;
            best = min(best, root[j]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if (lane == 0) labels[i] = best == INT_MAX ? -1 : cid[best];
}

struct Layout {
    size_t adj, norms, parent, root, cid, corebits, total;
};

Layout layout(int64_t n, int E) {
    const size_t W = (size_t)(n + 63) / 64;
    Carver c;
    Layout l;
    l.adj = c.take((size_t)E * (size_t)n * W * sizeof(u64));
    l.norms = c.take((size_t)n * sizeof(double));
    l.parent = c.take((size_t)n * sizeof(int32_t));
    l.root = c.take((size_t)n * sizeof(int32_t));
    l.cid = c.take((size_t)n * sizeof(int32_t));
    l.corebits = c.take(W * sizeof(u64));
    l.total = c.off;
    return l;
}

constexpr int64_t kMaxN = 262144;   // 4096 x 4096 tiles of 256 threads: the launch stays below 2^32 threads

}  // namespace

namespace dbscan {

size_t workspace(int64_t n, int E) {
    if (n < 1 || n > kMaxN || E < 1 || E > kMaxRadii) return 0;
    return layout(n, E).total;
}

int neighbors(hipStream_t s, const float* X, int64_t n, int d, const double* radii_sq, int E, int32_t* counts,
              uint64_t* borderline, void* ws, size_t ws_bytes) {
    HLMC_CHECK_ARG(X && radii_sq && counts && borderline && ws, "dbscan_neighbors: NULL argument");
    HLMC_CHECK_ARG(n >= 1 && n <= kMaxN && d >= 1, "dbscan_neighbors: need 1 <= n <= 262144 and d >= 1");
    HLMC_CHECK_ARG(E >= 1 && E <= kMaxRadii, "dbscan_neighbors: need 1 <= E <= 32 radii per call");
    for (int e = 0; e < E; ++e)
        HLMC_CHECK_ARG(radii_sq[e] >= 0.0, "dbscan_neighbors: squared radius must be >= 0 (and not NaN)");
    const Layout l = layout(n, E);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "dbscan_neighbors: workspace too small (hlmc_dbscan_workspace)");
    char* w = static_cast<char*>(ws);
    u64* adj = reinterpret_cast<u64*>(w + l.adj);
    double* norms = reinterpret_cast<double*>(w + l.norms);
    const int64_t W = (n + 63) / 64;
    Radii R;
    for (int e = 0; e < kMaxRadii; ++e) R.r[e] = e < E ? radii_sq[e] : 0.0;
    const double tolc = 4.0 * (double)(d + 4) * 0x1p-53;
    HLMC_HIP(hipMemsetAsync(borderline, 0, (size_t)E * sizeof(uint64_t), s));
    db_norms_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(X, n, d, norms);
    HLMC_LAUNCHED();
    const dim3 grid((unsigned)W, (unsigned)((n + kTile - 1) / kTile));
    db_neigh_kernel<<<grid, 256, 0, s>>>(X, norms, n, d, R, E, tolc, adj, W, reinterpret_cast<u64*>(borderline));
    HLMC_LAUNCHED();
    const int64_t rows = (int64_t)E * n;
    db_count_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(adj, n, W, E, counts);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int labels(hipStream_t s, int64_t n, int E, int e, int min_samples, const int32_t* counts, void* ws, size_t ws_bytes,
           int32_t* labels_out, uint8_t* core_out, int32_t* n_clusters) {
    HLMC_CHECK_ARG(counts && ws && labels_out && core_out, "dbscan_labels: NULL argument");
    HLMC_CHECK_ARG(n >= 1 && n <= kMaxN, "dbscan_labels: need 1 <= n <= 262144");
    HLMC_CHECK_ARG(E >= 1 && E <= kMaxRadii && e >= 0 && e < E, "dbscan_labels: need 1 <= E <= 32 and 0 <= e < E");
    HLMC_CHECK_ARG(min_samples >= 1, "dbscan_labels: min_samples must be >= 1");
    const Layout l = layout(n, E);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "dbscan_labels: workspace too small (hlmc_dbscan_workspace)");
    char* w = static_cast<char*>(ws);
    const int64_t W = (n + 63) / 64;
    const u64* adj = reinterpret_cast<const u64*>(w + l.adj) + (size_t)e * (size_t)n * (size_t)W;
    int32_t* parent = reinterpret_cast<int32_t*>(w + l.parent);
    int32_t* root = reinterpret_cast<int32_t*>(w + l.root);
    int32_t* cid = reinterpret_cast<int32_t*>(w + l.cid);
    u64* corebits = reinterpret_cast<u64*>(w + l.corebits);
    const int32_t* cnt = counts + (size_t)e * (size_t)n;
    const unsigned per_thread = (unsigned)((W * 64 + 255) / 256), per_wave = (unsigned)((n + 3) / 4);
    db_core_kernel<<<per_thread, 256, 0, s>>>(cnt, n, min_samples, core_out, corebits, parent);
    HLMC_LAUNCHED();
    db_union_kernel<<<per_wave, 256, 0, s>>>(adj, n, W, core_out, corebits, parent);
    HLMC_LAUNCHED();
    db_flatten_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(parent, n, core_out, root);
    HLMC_LAUNCHED();
    db_number_kernel<<<1, 1024, 0, s>>>(root, n, cid, n_clusters);
    HLMC_LAUNCHED();
    db_label_kernel<<<per_wave, 256, 0, s>>>(adj, n, W, core_out, corebits, root, cid, labels_out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

}  // namespace dbscan
}  // namespace hlmc
