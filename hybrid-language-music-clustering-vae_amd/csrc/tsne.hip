// t-SNE on the GPU (sklearn.manifold.TSNE at src/Simple_VAE.py:302-303, src/Convolutional_VAE.py:468-469 and
// src/Conditional_VAE.py:515-517): sklearn's method='barnes_hut' objective -- a sparse kNN affinity matrix P and a
// Student-t Q -- with the repulsive sum and Z taken over all pairs, which is what sklearn computes at angle = 0
// (DESIGN.md §12).  Four stages, every sum in an order that depends on the sizes alone, integer atomics only:
//
// knn         float64 squared distances |x_i|^2 + |x_j|^2 - 2 x_i.x_j on the tile of f64tile.hpp, one chunk of rows at
//             a time into a slab of the workspace (self = +inf); per row an 8 x 8-bit radix select of the k-th smallest
//             bit pattern, the candidates compacted into LDS and sorted there by (distance, index).
// affinities  sklearn's perplexity search, one wave per row (lane l holds neighbours l, l + 64, ..., added in that
//             order and then by the xor butterfly 32, 16, .., 1); P + P^T over the union pattern (without exact zeros, as scipy) by count, scan,
//             fill and a rank placement per row (columns ascending); the total in a fixed order; float32 values.
// gradient    repulsion over (256-row block x column slab) with the slab's y staged through LDS, float32 pair
//             arithmetic, float64 accumulators, slab partials added in slab order; attraction one wave per CSR row.
// run         n_iter iterations of sklearn's _gradient_descent update, gradient included, without a host sync.
//
// Built with -ffp-contract=off: the float32 pair arithmetic and the update are what tests/tsne_check.py restates
// operation by operation.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "f64tile.hpp"
#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

using namespace f64tile;
typedef unsigned long long u64;

constexpr int64_t kMaxN = 131072;
constexpr int kMaxD = 4096;
constexpr int kMaxK = 512;
constexpr int64_t kSlabBytes = (int64_t)1 << 28;   // the kNN distance slab: at most 256 MiB
constexpr int kRowBlock = 256;                     // rows of a repulsion block (one per thread)
constexpr int kColSlabMin = 256;                   // shortest column slab = columns staged per LDS fill
constexpr int kColSlabsMax = 64;                   // most column slabs
constexpr double kEpsDbl = 2.220446049250313e-16;  // numpy.finfo(double).eps: sklearn's MACHINE_EPSILON
constexpr double kTiny32 = 1.1754943508222875e-38; // numpy.finfo(float32).tiny: the clamp of sklearn's KL terms

// rows of a kNN chunk: a function of n alone
int64_t knn_chunk_rows(int64_t n) {
    const int64_t fit = kSlabBytes / (8 * n) / kTile * kTile;
    const int64_t all = (n + kTile - 1) / kTile * kTile;
    return std::min(all, std::max<int64_t>(kTile, fit));
}

// columns of a repulsion slab: a function of n alone
int64_t col_slab_len(int64_t n) {
    const int64_t per = (n + kColSlabsMax - 1) / kColSlabsMax;
    return std::max<int64_t>(kColSlabMin, (per + kColSlabMin - 1) / kColSlabMin * kColSlabMin);
}

// The gradient's buffers come first and depend on n alone, so hlmc_tsne_gradient / _run accept a workspace sized for
// any (d, k); the kNN and affinity buffers follow.
struct Layout {
    int64_t col_slab, col_slabs, chunk_rows;
    size_t part, rep, rowstat, grad, grad_total;
    size_t norms, slab, extra, cursor, tmp_col, tmp_val, sorted_val, rowsum, total_p, total;
};

Layout layout(int64_t n, int d, int k) {
    Layout l;
    l.col_slab = col_slab_len(n);
    l.col_slabs = (n + l.col_slab - 1) / l.col_slab;
    l.chunk_rows = knn_chunk_rows(n);
    const size_t nn = (size_t)n, cap = 2 * nn * (size_t)k;
    Carver c;
    l.part = c.take((size_t)l.col_slabs * 3 * nn * sizeof(double));
    l.rep = c.take(3 * nn * sizeof(double));
    l.rowstat = c.take(2 * nn * sizeof(double));
    l.grad = c.take(2 * nn * sizeof(float));
    l.grad_total = c.off;
    l.norms = c.take(nn * sizeof(double));
    l.slab = c.take((size_t)l.chunk_rows * nn * sizeof(double));
    l.extra = c.take(nn * sizeof(int32_t));
    l.cursor = c.take(nn * sizeof(int32_t));
    l.tmp_col = c.take(cap * sizeof(int32_t));
    l.tmp_val = c.take(cap * sizeof(double));
    l.sorted_val = c.take(cap * sizeof(double));
    l.rowsum = c.take(nn * sizeof(double));
    l.total_p = c.take(sizeof(double));
    l.total = c.off;
    return l;
}

bool sizes_ok(int64_t n, int d, int k) {
    return n >= 2 && n <= kMaxN && d >= 1 && d <= kMaxD && k >= 1 && k <= kMaxK && k <= n - 1;
}

// sum of x[0 .. n) by one block of 256 threads: thread t adds x[t], x[t + 256], ... in that order, then the LDS tree
// 128, 64, .., 1 (sh[t] += sh[t + s]).  Every thread returns the total.
__device__ __forceinline__ double block_sum_ordered(const double* __restrict__ x, int64_t n, double* sh) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += x[i];
    __syncthreads();
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    return sh[0];
}

// ------------------------------------------------------------------------------------------------ kNN
__global__ __launch_bounds__(256) void tsne_norms_kernel(const float* __restrict__ X, int64_t n, int d,
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

// slab[(i - r0)][j] = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j), +inf on the diagonal, for the chunk's rows i < n, j < n
__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ X, const double* __restrict__ norms,
                                                        int64_t n, int d, int64_t r0, double* __restrict__ slab) {
    __shared__ double a_sh[RowImage::kDoubles];
    __shared__ double b_sh[RowImage::kDoubles];
    const RowImage As{a_sh}, Bs{b_sh};
    const int64_t i0 = r0 + (int64_t)blockIdx.y * kTile, j0 = (int64_t)blockIdx.x * kTile;
    if (i0 >= n) return;   // block-uniform
    double4_t acc[4] = {};
    Stage<RowImage, float> pa, pb;
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
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t gi = i0 + acc_row(q);
        if (gi >= n) continue;
        const double ni = norms[gi];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t gj = j0 + acc_col(t);
            if (gj >= n) continue;
            const double v = fmax(0.0, (ni + norms[gj]) - 2.0 * acc[t][q]) + 0.0;   // + 0.0: never the pattern of -0.0
            slab[(size_t)(gi - r0) * (size_t)n + (size_t)gj] = gi == gj ? __builtin_inf() : v;
        }
    }
}

// One block per row of the chunk: the k smallest (distance, index) pairs, ascending.
__global__ __launch_bounds__(256) void tsne_select_kernel(const double* __restrict__ slab, int64_t n, int k,
                                                          int64_t r0, int32_t* __restrict__ out_idx,
                                                          double* __restrict__ out_d2) {
    __shared__ int hist[256];
    __shared__ u64 key[kMaxK];
    __shared__ int id[kMaxK];
    __shared__ int wtot[4];
    __shared__ int counter;
    const int64_t row = r0 + blockIdx.x;
    if (row >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64* bits = reinterpret_cast<const u64*>(slab + (size_t)blockIdx.x * (size_t)n);
    // radix select, 8 bits a pass from the top: non-negative doubles order as their bit patterns
    u64 prefix = 0, mask = 0;
    int want = k;   // rank (1-based) of the wanted element among those that match the prefix
    int eq_count = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int64_t j = tid; j < n; j += 256) {
            const u64 b = bits[j];
            if ((b & mask) == prefix) atomicAdd(&hist[(int)((b >> shift) & 0xff)], 1);
        }
        __syncthreads();
        int acc = 0, digit = 0;
        for (; digit < 256; ++digit) {   // every thread walks the same histogram: uniform result
            const int h = hist[digit];
            if (acc + h >= want) break;
            acc += h;
        }
        digit = min(digit, 255);   // unreachable: want never exceeds the elements that match the prefix
        want -= acc;
        eq_count = hist[digit];
        prefix |= (u64)digit << shift;
        mask |= (u64)0xff << shift;
        __syncthreads();
    }
    // prefix = the k-th smallest pattern T; `want` of the eq_count elements equal to T are taken, lowest index first
    for (int t = tid; t < kMaxK; t += 256) {
        key[t] = ~(u64)0;
        id[t] = INT32_MAX;
    }
    if (tid == 0) counter = 0;
    __syncthreads();
    const bool all_equal_taken = want == eq_count;
    for (int64_t j = tid; j < n; j += 256) {
        const u64 b = bits[j];
        if (b < prefix || (all_equal_taken && b == prefix)) {
            const int slot = atomicAdd(&counter, 1);   // the slot order is arbitrary: the sort below removes it
            if (slot < kMaxK) {
                key[slot] = b;
                id[slot] = (int)j;
            }
        }
    }
    __syncthreads();
    if (!all_equal_taken) {
        int base = counter;        // k - want entries so far
        int taken = 0;             // equal elements taken so far (uniform)
        for (int64_t j0 = 0; j0 < n && taken < want; j0 += 256) {
            const int64_t j = j0 + tid;
            const bool eq = j < n && bits[j] == prefix;
            const u64 bal = __ballot(eq);
            if (lane == 0) wtot[wv] = __popcll(bal);
            __syncthreads();
            int before = __popcll(bal & (((u64)1 << lane) - 1));
            for (int w = 0; w < wv; ++w) before += wtot[w];
            const int chunk_total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
            if (eq && taken + before < want) {
                const int slot = base + taken + before;
                if (slot < kMaxK) {
                    key[slot] = prefix;
                    id[slot] = (int)j;
                }
            }
            taken += chunk_total;
            __syncthreads();
        }
    }
    __syncthreads();
    // bitonic sort of the 512 (key, id) slots, ascending; the padding sorts last
    for (int size = 2; size <= kMaxK; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < kMaxK / 2; t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 ka = key[lo], kb = key[hi];
                const int ia = id[lo], ib = id[hi];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == up) {
                    key[lo] = kb;
                    key[hi] = ka;
                    id[lo] = ib;
                    id[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < k; t += 256) {
        out_idx[(size_t)row * k + t] = id[t];
        out_d2[(size_t)row * k + t] = __longlong_as_double((long long)key[t]);
    }
}

// ------------------------------------------------------------------------------------------------ affinities
// sklearn's _binary_search_perplexity on row i, one wave per row.  Every lane holds the same sums (the xor butterfly
// adds the same pairs in every lane), so the branches are wave-uniform.
__global__ __launch_bounds__(256) void tsne_search_kernel(const double* __restrict__ d2, int64_t n, int k,
                                                          double desired_entropy, double* __restrict__ beta_out,
                                                          double* __restrict__ cond_p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    constexpr int kPerLane = kMaxK / 64;
    double dist[kPerLane], p[kPerLane];
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) {
        const int j = lane + 64 * u;
        dist[u] = j < k ? (double)(float)d2[(size_t)row * k + j] : 0.0;   // sklearn searches on the float32 distances
        p[u] = 0.0;
    }
    double beta = 1.0, beta_min = -__builtin_inf(), beta_max = __builtin_inf();
    for (int step = 0; step < 100; ++step) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u)
            if (lane + 64 * u < k) {
                p[u] = exp(-dist[u] * beta);
                s += p[u];
            }
        s = wave_sum(s);
        if (s == 0.0) s = (double)1e-8f;   // sklearn's EPSILON_DBL is a C float
        double sd = 0.0;
#pragma unroll
        for (int u = 0; u < kPerLane; ++u)
            if (lane + 64 * u < k) {
                p[u] /= s;
                sd += dist[u] * p[u];
            }
        sd = wave_sum(sd);
        const double diff = (log(s) + beta * sd) - desired_entropy;
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == __builtin_inf() ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -__builtin_inf() ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    if (lane == 0) beta_out[row] = beta;
#pragma unroll
    for (int u = 0; u < kPerLane; ++u)
        if (lane + 64 * u < k) cond_p[(size_t)row * k + lane + 64 * u] = p[u];
}

// position of j among row i's neighbours, or -1
__device__ __forceinline__ int find_neighbor(const int32_t* __restrict__ idx, int k, int64_t i, int j) {
    const int32_t* r = idx + (size_t)i * k;
    for (int s = 0; s < k; ++s)
        if (r[s] == j) return s;
    return -1;
}

// The value of the pair (j, i = idx[j][t]) in P + P^T and whether i lists j as well.  p_ji + p_ij is commutative, so
// both rows compute the same bits; an entry without a partner is the conditional value itself.
__device__ __forceinline__ double pair_value(const int32_t* __restrict__ idx, const double* __restrict__ cond_p, int k,
                                             int64_t j, int i, int64_t e, bool& mutual) {
    const int s = find_neighbor(idx, k, i, (int)j);
    mutual = s >= 0;
    return mutual ? cond_p[e] + cond_p[(size_t)i * k + s] : cond_p[e];
}

// cnt[i] = stored entries of row i: its own neighbours plus the rows that list i while i does not list them, without
// the entries whose value is exactly 0 (an underflowed exp), which scipy's P + P.T drops as well
__global__ __launch_bounds__(256) void tsne_count_kernel(const int32_t* __restrict__ idx,
                                                         const double* __restrict__ cond_p, int64_t n, int k,
                                                         int32_t* __restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const int64_t j = e / k;
    const int i = idx[e];
    bool mutual;
    if (pair_value(idx, cond_p, k, j, i, e, mutual) == 0.0) return;
    atomicAdd(&cnt[j], 1);
    if (!mutual) atomicAdd(&cnt[i], 1);
}

// indptr[0] = 0, indptr[i + 1] = indptr[i] + cnt[i]; one block of 1024, thread t owns a contiguous run of rows
__global__ __launch_bounds__(1024) void tsne_scan_kernel(const int32_t* __restrict__ cnt, int64_t n,
                                                         int64_t* __restrict__ indptr) {
    __shared__ int64_t run[1024];
    const int64_t per = (n + 1023) / 1024;
    const int64_t a = min(n, (int64_t)threadIdx.x * per), b = min(n, a + per);
    int64_t s = 0;
    for (int64_t i = a; i < b; ++i) s += cnt[i];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int t = 0; t < 1024; ++t) {
            const int64_t v = run[t];
            run[t] = acc;
            acc += v;
        }
        indptr[0] = 0;
    }
    __syncthreads();
    s = run[threadIdx.x];
    for (int64_t i = a; i < b; ++i) {
        s += cnt[i];
        indptr[i + 1] = s;
    }
}

// The entries land in their rows in arrival order (integer cursors); tsne_place_kernel orders each row by column,
// which removes the arrival order from the result.
__global__ __launch_bounds__(256) void tsne_fill_kernel(const int32_t* __restrict__ idx,
                                                        const double* __restrict__ cond_p, int64_t n, int k,
                                                        const int64_t* __restrict__ indptr,
                                                        int32_t* __restrict__ cursor, int32_t* __restrict__ tmp_col,
                                                        double* __restrict__ tmp_val) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const int64_t j = e / k;
    const int i = idx[e];
    bool mutual;
    const double v = pair_value(idx, cond_p, k, j, i, e, mutual);
    if (v == 0.0) return;
    const int64_t own = indptr[j] + atomicAdd(&cursor[j], 1);
    tmp_col[own] = i;
    tmp_val[own] = v;
    if (!mutual) {
        const int64_t at = indptr[i] + atomicAdd(&cursor[i], 1);
        tmp_col[at] = (int)j;
        tmp_val[at] = v;
    }
}

// one block per row: an entry's slot is the number of smaller columns in its row (the columns of a row are distinct)
__global__ __launch_bounds__(256) void tsne_place_kernel(const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ tmp_col,
                                                         const double* __restrict__ tmp_val,
                                                         int32_t* __restrict__ indices,
                                                         double* __restrict__ sorted_val) {
    const int64_t lo = indptr[blockIdx.x], len = indptr[blockIdx.x + 1] - lo;
    for (int64_t e = threadIdx.x; e < len; e += 256) {
        const int c = tmp_col[lo + e];
        int64_t rank = 0;
        for (int64_t f = 0; f < len; ++f) rank += tmp_col[lo + f] < c ? 1 : 0;
        indices[lo + rank] = c;
        sorted_val[lo + rank] = tmp_val[lo + e];
    }
}

// rowsum[i] = the row's values added in column order by one thread
__global__ __launch_bounds__(256) void tsne_rowsum_kernel(const int64_t* __restrict__ indptr,
                                                          const double* __restrict__ sorted_val, int64_t n,
                                                          double* __restrict__ rowsum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s += sorted_val[e];
    rowsum[i] = s;
}

__global__ __launch_bounds__(256) void tsne_total_kernel(const double* __restrict__ rowsum, int64_t n,
                                                         double* __restrict__ total) {
    __shared__ double sh[256];
    const double s = block_sum_ordered(rowsum, n, sh);
    if (threadIdx.x == 0) total[0] = s;
}

__global__ __launch_bounds__(256) void tsne_normalize_kernel(const int64_t* __restrict__ indptr, int64_t n,
                                                             const double* __restrict__ sorted_val,
                                                             const double* __restrict__ total,
                                                             float* __restrict__ values) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= indptr[n]) return;
    values[e] = (float)(sorted_val[e] / fmax(total[0], kEpsDbl));
}

// ------------------------------------------------------------------------------------------------ gradient
// part[slab][c][i], c = 0: sum_j q_ij^2 (y_i0 - y_j0), 1: the same for coordinate 1, 2: sum_j q_ij, over the slab's
// columns j != i in ascending order; q_ij = rcp(1 + (dx dx + dy dy)) in float32, each term widened and added in float64.
__global__ __launch_bounds__(256) void tsne_repulsion_kernel(const float2* __restrict__ Y, int64_t n, int64_t slab,
                                                             double* __restrict__ part) {
    __shared__ float2 ys[kColSlabMin];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kRowBlock + tid;
    const float2 yi = i < n ? Y[i] : make_float2(0.f, 0.f);
    const int64_t j0 = (int64_t)blockIdx.y * slab, j1 = min(n, j0 + slab);
    double fx = 0.0, fy = 0.0, sq = 0.0;
    for (int64_t c0 = j0; c0 < j1; c0 += kColSlabMin) {
        __syncthreads();
        ys[tid] = c0 + tid < j1 ? Y[c0 + tid] : make_float2(0.f, 0.f);
        __syncthreads();
        const int cnt = (int)min((int64_t)kColSlabMin, j1 - c0);
        const int self = (int)(i - c0);   // the row's own column inside this fill, if 0 <= self < cnt
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {
            const float2 yj = ys[t];      // every lane reads the same address: an LDS broadcast
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float d2 = dx * dx + dy * dy;
            float q = __builtin_amdgcn_rcpf(1.0f + d2);
            q = t == self ? 0.f : q;
            const float q2 = q * q;
            sq += (double)q;
            fx += (double)(q2 * dx);
            fy += (double)(q2 * dy);
        }
    }
    if (i < n) {
        double* p = part + (size_t)blockIdx.y * 3 * (size_t)n;
        p[i] = fx;
        p[(size_t)n + i] = fy;
        p[2 * (size_t)n + i] = sq;
    }
}

// rep[c][i] = part[0][c][i] + part[1][c][i] + ... in slab order
__global__ __launch_bounds__(256) void tsne_slabsum_kernel(const double* __restrict__ part, int64_t n, int64_t slabs,
                                                           double* __restrict__ rep) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * n) return;
    double s = 0.0;
    for (int64_t b = 0; b < slabs; ++b) s += part[(size_t)b * 3 * (size_t)n + e];
    rep[e] = s;
}

__global__ __launch_bounds__(256) void tsne_z_kernel(const double* __restrict__ rep, int64_t n,
                                                     double* __restrict__ stats) {
    __shared__ double sh[256];
    const double z = block_sum_ordered(rep + 2 * (size_t)n, n, sh);
    if (threadIdx.x == 0) stats[0] = z;
}

// One wave per row: the attractive sum over the row's stored entries (lane l takes entries l, l + 64, ... in that
// order, then the xor butterfly), in float64; grad = 4 (exaggeration attr - rep / Z) rounded once to float32.
__global__ __launch_bounds__(256) void tsne_attract_kernel(const float2* __restrict__ Y, int64_t n,
                                                           const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const float* __restrict__ values, double exaggeration,
                                                           const double* __restrict__ rep,
                                                           const double* __restrict__ stats, int want_stats,
                                                           float2* __restrict__ grad, double* __restrict__ rowstat) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double z = fmax(stats[0], kEpsDbl);   // sklearn: sum_Q = max(sum_Q, FLOAT64_EPS)
    const float2 yi = Y[i];
    const double yx = (double)yi.x, yy = (double)yi.y;
    double ax = 0.0, ay = 0.0, kl = 0.0;
    for (int64_t e = indptr[i] + lane; e < indptr[i + 1]; e += 64) {
        const float2 yj = Y[indices[e]];
        const double p = exaggeration * (double)values[e];
        const double dx = yx - (double)yj.x, dy = yy - (double)yj.y;
        const double q = 1.0 / (1.0 + (dx * dx + dy * dy));
        const double pq = p * q;
        ax += pq * dx;
        ay += pq * dy;
        if (want_stats) kl += p * log(fmax(p, kTiny32) / fmax(q / z, kTiny32));
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (want_stats) kl = wave_sum(kl);
    if (lane == 0) {
        const float gx = (float)(4.0 * (ax - rep[i] / z));
        const float gy = (float)(4.0 * (ay - rep[(size_t)n + i] / z));
        grad[i] = make_float2(gx, gy);
        if (want_stats) {
            rowstat[i] = kl;
            rowstat[(size_t)n + i] = (double)gx * (double)gx + (double)gy * (double)gy;
        }
    }
}

// stats[1] = KL, stats[2] = |grad|_2
__global__ __launch_bounds__(256) void tsne_stats_kernel(const double* __restrict__ rowstat, int64_t n,
                                                         double* __restrict__ stats) {
    __shared__ double sh[256];
    const double kl = block_sum_ordered(rowstat, n, sh);
    const double g2 = block_sum_ordered(rowstat + (size_t)n, n, sh);
    if (threadIdx.x == 0) {
        stats[1] = kl;
        stats[2] = sqrt(g2);
    }
}

// sklearn's _gradient_descent update in float32, element by element
__global__ __launch_bounds__(256) void tsne_update_kernel(float* __restrict__ Y, float* __restrict__ update,
                                                          float* __restrict__ gains, const float* __restrict__ grad,
                                                          int64_t n2, float momentum, float lr) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n2) return;
    const float g = grad[e], u = update[e];
    float ga = gains[e];
    ga = u * g < 0.0f ? ga + 0.2f : ga * 0.8f;
    ga = fmaxf(ga, 0.01f);
    const float un = momentum * u - lr * (g * ga);
    gains[e] = ga;
    update[e] = un;
    Y[e] = Y[e] + un;
}

int launch_gradient(hipStream_t s, const Layout& l, const float* Y, int64_t n, const int64_t* indptr,
                    const int32_t* indices, const float* values, double exaggeration, float* grad, double* stats,
                    int want_stats, char* w) {
    double* part = reinterpret_cast<double*>(w + l.part);
    double* rep = reinterpret_cast<double*>(w + l.rep);
    double* rowstat = reinterpret_cast<double*>(w + l.rowstat);
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const dim3 grid((unsigned)((n + kRowBlock - 1) / kRowBlock), (unsigned)l.col_slabs);
    tsne_repulsion_kernel<<<grid, 256, 0, s>>>(Y2, n, l.col_slab, part);
    HLMC_LAUNCHED();
    tsne_slabsum_kernel<<<(unsigned)((3 * n + 255) / 256), 256, 0, s>>>(part, n, l.col_slabs, rep);
    HLMC_LAUNCHED();
    tsne_z_kernel<<<1, 256, 0, s>>>(rep, n, stats);
    HLMC_LAUNCHED();
    tsne_attract_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(Y2, n, indptr, indices, values, exaggeration, rep, stats,
                                                               want_stats, reinterpret_cast<float2*>(grad), rowstat);
    HLMC_LAUNCHED();
    if (want_stats) {
        tsne_stats_kernel<<<1, 256, 0, s>>>(rowstat, n, stats);
        HLMC_LAUNCHED();
    }
    return HLMC_OK;
}

}  // namespace

namespace tsne {

size_t workspace(int64_t n, int d, int k) {
    if (!sizes_ok(n, d, k)) return 0;
    return layout(n, d, k).total;
}

int knn(hipStream_t s, const float* X, int64_t n, int d, int k, int32_t* nbr_idx, double* nbr_d2, void* ws,
        size_t ws_bytes) {
    HLMC_CHECK_ARG(X && nbr_idx && nbr_d2 && ws, "tsne_knn: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "tsne_knn: need 2 <= n <= 131072");
    HLMC_CHECK_ARG(d >= 1 && d <= kMaxD, "tsne_knn: need 1 <= d <= 4096");
    HLMC_CHECK_ARG(k >= 1 && k <= kMaxK && k <= n - 1, "tsne_knn: need 1 <= k <= min(512, n - 1)");
    const Layout l = layout(n, d, k);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "tsne_knn: workspace too small (hlmc_tsne_workspace)");
    char* w = static_cast<char*>(ws);
    double* norms = reinterpret_cast<double*>(w + l.norms);
    double* slab = reinterpret_cast<double*>(w + l.slab);
    tsne_norms_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(X, n, d, norms);
    HLMC_LAUNCHED();
    for (int64_t r0 = 0; r0 < n; r0 += l.chunk_rows) {
        const int64_t rows = std::min(l.chunk_rows, n - r0);
        const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile));
        tsne_dist_kernel<<<grid, 256, 0, s>>>(X, norms, n, d, r0, slab);
        HLMC_LAUNCHED();
        tsne_select_kernel<<<(unsigned)rows, 256, 0, s>>>(slab, n, k, r0, nbr_idx, nbr_d2);
        HLMC_LAUNCHED();
    }
    return HLMC_OK;
}

int affinities(hipStream_t s, const int32_t* nbr_idx, const double* nbr_d2, int64_t n, int k, double perplexity,
               double* beta, double* cond_p, int64_t* indptr, int32_t* indices, float* values, void* ws,
               size_t ws_bytes) {
    HLMC_CHECK_ARG(nbr_idx && nbr_d2 && beta && cond_p && indptr && indices && values && ws,
                   "tsne_affinities: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "tsne_affinities: need 2 <= n <= 131072");
    HLMC_CHECK_ARG(k >= 1 && k <= kMaxK && k <= n - 1, "tsne_affinities: need 1 <= k <= min(512, n - 1)");
    HLMC_CHECK_ARG(perplexity > 0.0 && std::isfinite(perplexity), "tsne_affinities: need a finite perplexity > 0");
    const Layout l = layout(n, 1, k);
    HLMC_CHECK_ARG(ws_bytes >= l.total, "tsne_affinities: workspace too small (hlmc_tsne_workspace)");
    char* w = static_cast<char*>(ws);
    int32_t* extra = reinterpret_cast<int32_t*>(w + l.extra);
    int32_t* cursor = reinterpret_cast<int32_t*>(w + l.cursor);
    int32_t* tmp_col = reinterpret_cast<int32_t*>(w + l.tmp_col);
    double* tmp_val = reinterpret_cast<double*>(w + l.tmp_val);
    double* sorted_val = reinterpret_cast<double*>(w + l.sorted_val);
    double* rowsum = reinterpret_cast<double*>(w + l.rowsum);
    double* total = reinterpret_cast<double*>(w + l.total_p);
    // sklearn passes the perplexity to its search as a C float
    const double desired = std::log((double)(float)perplexity);
    const unsigned per_entry = (unsigned)((n * k + 255) / 256);
    tsne_search_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(nbr_d2, n, k, desired, beta, cond_p);
    HLMC_LAUNCHED();
    HLMC_HIP(hipMemsetAsync(extra, 0, (l.cursor - l.extra) + (size_t)n * sizeof(int32_t), s));   // counts and cursors
    tsne_count_kernel<<<per_entry, 256, 0, s>>>(nbr_idx, cond_p, n, k, extra);
    HLMC_LAUNCHED();
    tsne_scan_kernel<<<1, 1024, 0, s>>>(extra, n, indptr);
    HLMC_LAUNCHED();
    tsne_fill_kernel<<<per_entry, 256, 0, s>>>(nbr_idx, cond_p, n, k, indptr, cursor, tmp_col, tmp_val);
    HLMC_LAUNCHED();
    tsne_place_kernel<<<(unsigned)n, 256, 0, s>>>(indptr, tmp_col, tmp_val, indices, sorted_val);
    HLMC_LAUNCHED();
    tsne_rowsum_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(indptr, sorted_val, n, rowsum);
    HLMC_LAUNCHED();
    tsne_total_kernel<<<1, 256, 0, s>>>(rowsum, n, total);
    HLMC_LAUNCHED();
    tsne_normalize_kernel<<<(unsigned)((2 * n * k + 255) / 256), 256, 0, s>>>(indptr, n, sorted_val, total, values);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int gradient(hipStream_t s, const float* Y, int64_t n, const int64_t* indptr, const int32_t* indices,
             const float* values, double exaggeration, float* grad, double* stats, int want_stats, void* ws,
             size_t ws_bytes) {
    HLMC_CHECK_ARG(Y && indptr && indices && values && grad && stats && ws, "tsne_gradient: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "tsne_gradient: need 2 <= n <= 131072");
    HLMC_CHECK_ARG(exaggeration > 0.0 && std::isfinite(exaggeration), "tsne_gradient: need a finite exaggeration > 0");
    const Layout l = layout(n, 1, 1);
    HLMC_CHECK_ARG(ws_bytes >= l.grad_total, "tsne_gradient: workspace too small (hlmc_tsne_workspace)");
    return launch_gradient(s, l, Y, n, indptr, indices, values, exaggeration, grad, stats, want_stats,
                           static_cast<char*>(ws));
}

int run(hipStream_t s, float* Y, float* update, float* gains, int64_t n, const int64_t* indptr,
        const int32_t* indices, const float* values, double exaggeration, double momentum, double learning_rate,
        int n_iter, double* stats, void* ws, size_t ws_bytes) {
    HLMC_CHECK_ARG(Y && update && gains && indptr && indices && values && stats && ws, "tsne_run: NULL argument");
    HLMC_CHECK_ARG(n >= 2 && n <= kMaxN, "tsne_run: need 2 <= n <= 131072");
    HLMC_CHECK_ARG(exaggeration > 0.0 && std::isfinite(exaggeration), "tsne_run: need a finite exaggeration > 0");
    HLMC_CHECK_ARG(momentum >= 0.0 && momentum < 1.0, "tsne_run: need 0 <= momentum < 1");
    HLMC_CHECK_ARG(learning_rate > 0.0 && std::isfinite(learning_rate), "tsne_run: need a finite learning_rate > 0");
    HLMC_CHECK_ARG(n_iter >= 1 && n_iter <= 100000, "tsne_run: need 1 <= n_iter <= 100000");
    const Layout l = layout(n, 1, 1);
    HLMC_CHECK_ARG(ws_bytes >= l.grad_total, "tsne_run: workspace too small (hlmc_tsne_workspace)");
    char* w = static_cast<char*>(ws);
    float* grad = reinterpret_cast<float*>(w + l.grad);
    for (int it = 0; it < n_iter; ++it) {
        HLMC_TRY(launch_gradient(s, l, Y, n, indptr, indices, values, exaggeration, grad, stats, it == n_iter - 1, w));
        tsne_update_kernel<<<(unsigned)((2 * n + 255) / 256), 256, 0, s>>>(Y, update, gains, grad, 2 * n,
                                                                          (float)momentum, (float)learning_rate);
        HLMC_LAUNCHED();
    }
    return HLMC_OK;
}

}  // namespace tsne
}  // namespace hlmc
