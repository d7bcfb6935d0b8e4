// K-Means device kernels with sklearn 1.7.2 (lloyd, dense float32) numerics, driven by the Python
// KMeans host (hybrid-language-music-clustering-vae_amd/cluster.py).  Reference call sites:
// src/Convolutional_VAE.py:317-319,379-380; src/Conditional_VAE.py:293-295,528; src/Simple_VAE.py:244-261.
//
// Order-sensitive float32 sums are evaluated in sklearn's single-thread order (sequential over rows)
// so labels and centres reproduce bit-for-bit whenever no distance is within rounding of a tie.
#include <algorithm>

#include "features.hpp"
#include "workspace.hpp"

namespace hlmc {
namespace {

__global__ void km_sub_kernel(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ mean,
                              float* __restrict__ Xc) {
    const int64_t tot = n * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x)
        Xc[i] = X[i] - mean[i % d];
}

// np.einsum("ij,ij->i") of one float64 row (sklearn row_norms on the upcast chunks): numpy's baseline-SSE2
// loop, 2 lanes, 8-element blocks added as 3, 2, 1, 0 with a separate multiply and add, then l0 + l1.
template <typename Ld>
__device__ __forceinline__ double einsum_sq_f64(Ld ld, int d) {
    double a0 = 0.0, a1 = 0.0;
    int i = 0;
    for (; d - i >= 8; i += 8)
        for (int t = 3; t >= 0; --t) {
            const double u = ld(i + 2 * t), v = ld(i + 2 * t + 1);
            a0 = u * u + a0;
            a1 = v * v + a1;
        }
    for (; i < d; i += 2) {
        const double u = ld(i), v = i + 1 < d ? ld(i + 1) : 0.0;
        a0 = u * u + a0;
        a1 = v * v + a1;
    }
    return a0 + a1;
}

// E-step, bit-exact to sklearn's lloyd_iter_chunked_dense (oracle/kmeans_oracle.py estep_dist):
//   ||c||^2: np.einsum row norms (4 lanes, 16-element blocks added as 3, 2, 1, 0, separate mul and add,
//            (l0 + l1) + (l2 + l3));
//   x.c:     OpenBLAS sgemm per 256-row chunk, column-major TN (M = k, N = chunk rows, K = d).  Small-matrix
//            kernel (M*N <= 1200, K >= 32, M*N*K <= 1e6): 16 lanes of fma over k = l (mod 16), reduced by an
//            adjacent-pair tree, or halves-first when the element lies in both remainders of 4; else one
//            sequential fma chain over k;
//   dist = ||c||^2 + (-2 * dot), first minimum.
// 4 threads per row (cluster j = part, part + 4, ...), 64 rows staged in LDS.  A block never straddles a
// 256-row chunk, so the small-kernel decision is block-uniform.
constexpr int kRows = 64;
constexpr int kChunk = 256;

__device__ __forceinline__ float km_tree_adjacent(float* a) {
#pragma unroll
    for (int w = 16; w > 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w / 2; ++i) a[i] = a[2 * i] + a[2 * i + 1];
    return a[0];
}
__device__ __forceinline__ float km_tree_halves(float* a) {
#pragma unroll
    for (int w = 16; w > 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w / 2; ++i) a[i] = a[i] + a[i + w / 2];
    return a[0];
}

// Restart-batched (blockIdx.y = restart r of R in lockstep, cluster.KMeans): centres C + r k d, labels / old +
// r n, n_changed + r; restarts outside the active mask are skipped.
__global__ __launch_bounds__(256) void km_assign_kernel(const float* __restrict__ X, int64_t n, int d,
                                                        const float* __restrict__ C, int k,
                                                        int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ old,
                                                        int32_t* __restrict__ n_changed, uint64_t active) {
    const int rs = blockIdx.y;
    if (!((active >> rs) & 1)) return;
    C += (int64_t)rs * k * d;
    labels += (int64_t)rs * n;
    if (old) old += (int64_t)rs * n;
    if (n_changed) n_changed += rs;
    extern __shared__ float smem[];
    const int ldc = d + 1;               // padded: the 4 centres a wave reads per c sit in distinct banks
    float* Cs = smem;                    // [k][d + 1]
    float* cn = Cs + k * ldc;            // [k] ||c||^2 (einsum order)
    float* Xs = cn + k;                  // [kRows][d + 1]
    const int ld = d + 1;
    for (int i = threadIdx.x; i < k * d; i += blockDim.x) Cs[(i / d) * ldc + i % d] = C[i];
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const float* cj = Cs + j * ldc;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int i = 0;
        for (; d - i >= 16; i += 16)
            for (int t = 3; t >= 0; --t)
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const float v = cj[i + 4 * t + l];
                    acc[l] = v * v + acc[l];
                }
        for (; i < d; i += 4)
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float v = i + l < d ? cj[i + l] : 0.f;
                acc[l] = v * v + acc[l];
            }
        cn[j] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    {
        // row-wise staging (no per-element division by d): wave w copies rows w, w + 4, ... lane-strided
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
        for (int rr = w; rr < kRows; rr += 4) {
            const bool ok = r0 + rr < n;
            const float* src = X + (ok ? r0 + rr : 0) * d;
            for (int c = l; c < d; c += 64) Xs[rr * ld + c] = ok ? src[c] : 0.f;
        }
    }
    __syncthreads();
    const int rr = threadIdx.x >> 2, part = threadIdx.x & 3;
    const int64_t row = r0 + rr;
    const int64_t cs = r0 / kChunk * kChunk;                      // this chunk's first row
    const int N = (int)min((int64_t)kChunk, n - cs);              // rows in the chunk (the last one is short)
    const bool small = (int64_t)k * N <= 1200 && d >= 32 && (double)k * N * d <= 1e6;
    const int jl = (int)(row - cs);
    const bool row_rem = jl >= 4 * (N / 4);
    const int k4 = 4 * (k / 4);
    const float* xr = Xs + rr * ld;
    float best = INFINITY;
    int bj = 0x7fffffff;
    auto consider = [&](int j, float dot) {
        const float dist = cn[j] + (-2.0f * dot);
        if (dist < best || (dist == best && j < bj)) { best = dist; bj = j; }
    };
    if (!small) {
        // regular kernel: sequential fma chains, up to 4 clusters interleaved per thread
        for (int j0 = part; j0 < k; j0 += 16) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const float* cp[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) cp[q] = Cs + min(j0 + 4 * q, k - 1) * ldc;
            for (int c = 0; c < d; ++c) {
                const float x = xr[c];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(x, cp[q][c], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + 4 * q < k) consider(j0 + 4 * q, acc[q]);
        }
    } else {
        for (int j = part; j < k; j += 4) {
            const float* cj = Cs + j * ldc;
            float a[16];
#pragma unroll
            for (int l = 0; l < 16; ++l) a[l] = 0.f;
            for (int b = 0; b < d; b += 16)
#pragma unroll
                for (int l = 0; l < 16; ++l)
                    if (b + l < d) a[l] = fmaf(xr[b + l], cj[b + l], a[l]);
            consider(j, (row_rem && j >= k4) ? km_tree_halves(a) : km_tree_adjacent(a));
        }
    }
    // combine the 4 partials (first minimum = smallest index among equal distances)
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (part == 0 && row < n) {
        labels[row] = bj;
        if (old && n_changed && old[row] != bj) atomicAdd(n_changed, 1);
    }
}

// sums[j][c] = sum_{i: l_i == j} X[i][c] in row order (float32); weight[j] = count.
// One wave per (64-column slab, cluster j).  The wave walks the labels in super-tiles of 1024 rows (16 per
// lane, the next super-tile prefetched into registers), compacts the rows of cluster j in row order with
// ballots into LDS, then gathers those rows' columns in groups of 64 (independent loads, all in flight)
// and adds them into one float32 accumulator per column in row order -- sklearn's single-thread order.
constexpr int kLabQ = 16;
constexpr int kSumGrp = 64;
template <bool kFull>
__device__ __forceinline__ float km_gather_add(const float* __restrict__ Xc, int d, const int* list, int g, int m,
                                               int lane, float s) {
    // one LDS read per 64 list entries; each row index is broadcast with readlane (no LDS round trip)
    const int mine = list[kFull ? g + lane : min(g + lane, m - 1)];
    float v[kSumGrp];
#pragma unroll
    for (int t = 0; t < kSumGrp; ++t) v[t] = Xc[(int64_t)__builtin_amdgcn_readlane(mine, t) * d];
#pragma unroll
    for (int t = 0; t < kSumGrp; ++t)
        if (kFull || g + t < m) s += v[t];
    return s;
}

__global__ __launch_bounds__(64) void km_sums_kernel(const float* __restrict__ X, int n, int d,
                                                     const int32_t* __restrict__ labels, int k,
                                                     float* __restrict__ sums, float* __restrict__ weight,
                                                     uint64_t active) {
    const int rs = blockIdx.z;   // restart (batched lockstep)
    if (!((active >> rs) & 1)) return;
    labels += (int64_t)rs * n;
    sums += (int64_t)rs * k * d;
    weight += (int64_t)rs * k;
    __shared__ int list[64 * kLabQ + kSumGrp];     // carried partial group + one super-tile of hits
    const int j = blockIdx.y;
    const int lane = threadIdx.x;
    const int c = blockIdx.x * 64 + lane;
    const float* __restrict__ Xc = X + (c < d ? c : d - 1);
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    float s = 0.f;
    int count = 0, p = 0;
    int lab[kLabQ], nxt[kLabQ];
    // rows past n read the last label (clamped, unconditional loads) and are masked out below
#pragma unroll
    for (int q = 0; q < kLabQ; ++q) lab[q] = labels[min(q * 64 + lane, n - 1)];
    for (int base = 0; base < n; base += 64 * kLabQ) {
        const int nb = base + 64 * kLabQ;
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) nxt[q] = labels[min(nb + q * 64 + lane, n - 1)];
        int tot = p;
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) {
            const int row = base + q * 64 + lane;
            const bool hit = lab[q] == j && row < n;
            const uint64_t mask = __ballot(hit);
            if (hit) list[tot + __popcll(mask & lt)] = row;
            tot += __popcll(mask);
        }
        __syncthreads();
        count += tot - p;
        int g = 0;
        for (; g + kSumGrp <= tot; g += kSumGrp) s = km_gather_add<true>(Xc, d, list, g, tot, lane, s);
        // carry the partial group (< 64 rows, row order kept) to the front of the list
        p = tot - g;
        const int carry = lane < p ? list[g + lane] : 0;
        __syncthreads();
        if (lane < p) list[lane] = carry;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) lab[q] = nxt[q];
    }
    if (p > 0) s = km_gather_add<false>(Xc, d, list, 0, p, lane, s);
    if (c < d) sums[(int64_t)j * d + c] = s;
    if (blockIdx.x == 0 && lane == 0) weight[j] = (float)count;
}

// ---- M-step via a stable partition of the rows by label (row order kept inside every cluster), then one
// block per (64-column slab, cluster) walking the cluster's contiguous row list.  The sum is a serial float32
// chain per column (sklearn's single-thread order), so the block is a producer/consumer ring: 15 loader waves
// gather 64-row chunks (one row per load instruction, 64 in flight per lane) into an 8-slot LDS ring and wave 0
// adds the slots in chunk order, handing slots back through LDS flags -- the add chain never waits on HBM.
constexpr int kPartTile = 1024;   // rows per partition tile (one wave, 16 chunks of 64)
// lanes holding the same label as this lane, from one ballot per label bit (no loop over the clusters)
__device__ __forceinline__ uint64_t km_same_label(int lab, int nbits, bool valid) {
    uint64_t eq = __ballot(valid);
    for (int bit = 0; bit < nbits; ++bit) {
        const uint64_t m = __ballot(valid && ((lab >> bit) & 1));
        eq &= ((lab >> bit) & 1) ? m : ~m;
    }
    return eq;
}
// One restart's partition workspace (int32): hist [tiles][k] | base [tiles][k] | off [k + 1] | order [n], packed, the
// total rounded to 256 bytes (the stride between restarts).
struct Layout { int tiles; size_t hist, base, off, order, total; };
Layout layout(int64_t n, int k) {
    Layout l;
    l.tiles = (int)((n + kPartTile - 1) / kPartTile);
    Carver c;
    l.hist = c.pack((size_t)l.tiles * k * sizeof(int));
    l.base = c.pack((size_t)l.tiles * k * sizeof(int));
    l.off = c.pack((size_t)(k + 1) * sizeof(int));
    l.order = c.pack((size_t)n * sizeof(int));
    l.total = align256(c.off);
    return l;
}
// restart-batched: each restart has its own labels [n] and its own Layout::total bytes of the workspace.  The device
// side walks the same packed order from (tiles, k) instead of carrying Layout's four offsets: with the offsets as
// kernel arguments km_ring_kernel's prologue is 24 bytes shorter, its loops sit elsewhere in their instruction
// cache lines, and the partitioned sums measured 3 % slower (profiles/r15/ab.txt).
struct PartWs {
    char* base;
    int64_t bytes;   // per restart: Layout::total
    int tiles, k;
    __device__ int* hist(int r) const { return reinterpret_cast<int*>(base + r * bytes); }
    __device__ int* bas(int r) const { return hist(r) + (int64_t)tiles * k; }
    __device__ int* off(int r) const { return bas(r) + (int64_t)tiles * k; }
    __device__ int* order(int r) const { return off(r) + (k + 1); }
};
// One wave's walk over partition tile blockIdx.x of one restart's labels: the tile's 16 x 64 labels are loaded (-1 past
// n), then, behind a barrier for the caller's LDS counters, each 64-row group in row order gets
// body(label, valid, lanes holding the same label, lanes below this one, row).
template <typename Body>
__device__ __forceinline__ void km_part_walk(const int32_t* __restrict__ labels, int n, int nbits, Body body) {
    const int lane = threadIdx.x, tile = blockIdx.x;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int lab[kPartTile / 64];
#pragma unroll
    for (int q = 0; q < kPartTile / 64; ++q) {
        const int row = tile * kPartTile + q * 64 + lane;
        lab[q] = row < n ? labels[row] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPartTile / 64; ++q) {
        const bool valid = lab[q] >= 0;
        body(lab[q], valid, km_same_label(lab[q], nbits, valid), lt, tile * kPartTile + q * 64 + lane);
    }
}
// hist[tile][c] = rows of cluster c in the tile; blockIdx.y = restart
__global__ __launch_bounds__(64) void km_part_hist_kernel(const int32_t* __restrict__ labels, int n, int k, int nbits,
                                                          PartWs pw, uint64_t active) {
    const int rs = blockIdx.y;
    if (!((active >> rs) & 1)) return;
    int* __restrict__ hist = pw.hist(rs);
    extern __shared__ int cnt[];  // [k]
    for (int c = threadIdx.x; c < k; c += 64) cnt[c] = 0;
    km_part_walk(labels + (int64_t)rs * n, n, nbits, [&](int lab, bool valid, uint64_t eq, uint64_t lt, int) {
        if (valid && (eq & lt) == 0) atomicAdd(&cnt[lab], __popcll(eq));   // one add per label, no return
    });
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += 64) hist[(int64_t)blockIdx.x * k + c] = cnt[c];
}
// base[tile][c] = (rows of clusters < c) + (rows of cluster c in tiles < tile); off[c] = first row of cluster c.
// 16 waves: per cluster a wave-level scan over the tiles (no block barriers inside), cluster totals in LDS.
template <typename V>
__device__ __forceinline__ V wave_incl_scan(V v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__global__ __launch_bounds__(1024) void km_part_scan_kernel(PartWs pw, uint64_t active) {
    const int rs = blockIdx.x;
    if (!((active >> rs) & 1)) return;
    const int tiles = pw.tiles, k = pw.k;
    const int* __restrict__ hist = pw.hist(rs);
    int* __restrict__ base = pw.bas(rs);
    int* __restrict__ off = pw.off(rs);
    extern __shared__ int tot[];  // [k + 1]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int c = wave; c < k; c += 16) {
        int run = 0;
        for (int t0 = 0; t0 < tiles; t0 += 64) {
            const int v = (t0 + lane < tiles) ? hist[(int64_t)(t0 + lane) * k + c] : 0;
            run += __shfl(wave_incl_scan(v, lane), 63, 64);
        }
        if (lane == 0) tot[c] = run;
    }
    __syncthreads();
    if (wave == 0) {   // exclusive scan of the cluster totals
        int run = 0;
        for (int c0 = 0; c0 < k; c0 += 64) {
            const int v = (c0 + lane < k) ? tot[c0 + lane] : 0;
            const int inc = wave_incl_scan(v, lane);
            if (c0 + lane < k) {
                off[c0 + lane] = run + inc - v;
                tot[c0 + lane] = run + inc - v;
            }
            run += __shfl(inc, 63, 64);
        }
        if (lane == 0) off[k] = run;
    }
    __syncthreads();
    for (int c = wave; c < k; c += 16) {
        int run = tot[c];
        for (int t0 = 0; t0 < tiles; t0 += 64) {
            const int v = (t0 + lane < tiles) ? hist[(int64_t)(t0 + lane) * k + c] : 0;
            const int inc = wave_incl_scan(v, lane);
            if (t0 + lane < tiles) base[(int64_t)(t0 + lane) * k + c] = run + inc - v;
            run += __shfl(inc, 63, 64);
        }
    }
}
// order[base[tile][c] + rank] = row, rank = rows of cluster c before it in the tile (ballot prefix, row order)
__global__ __launch_bounds__(64) void km_part_scatter_kernel(const int32_t* __restrict__ labels, int n, int k,
                                                             int nbits, PartWs pw, uint64_t active) {
    const int rs = blockIdx.y;
    if (!((active >> rs) & 1)) return;
    const int* __restrict__ base = pw.bas(rs);
    int* __restrict__ order = pw.order(rs);
    extern __shared__ int cur[];  // [k] next free position per cluster
    for (int c = threadIdx.x; c < k; c += 64) cur[c] = base[(int64_t)blockIdx.x * k + c];
    km_part_walk(labels + (int64_t)rs * n, n, nbits, [&](int lab, bool valid, uint64_t eq, uint64_t lt, int row) {
        const int b0 = valid ? cur[lab] : 0;
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): every lane's read of cur[] returned (one wave)
        if (valid && (eq & lt) == 0) cur[lab] = b0 + __popcll(eq);
        if (valid) order[b0 + __popcll(eq & lt)] = row;
    });
}
constexpr int kRingSlots = 8, kRingLoaders = 15, kRingPitch = 68;   // slot [column][row], rows padded to 68
__device__ __forceinline__ int lds_acquire(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_release(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// kMode 0: cluster j = blockIdx.y, entries order[off[j] .. off[j+1]) -> out0[j][c] = sum, out1[j] = count.
// kMode 1: all n rows in order, one pass (out1 == nullptr) or two -> out0[c] = X.mean(axis=0) and
// out1[c] = np.var(X, axis=0) (numpy: sequential float32 sums, / n; the second pass adds (x - mean)^2).
// kMode 0 is restart-batched: blockIdx.z = restart (order / off from its PartWs, out0 + r k d, out1 + r k)
template <int kMode>
__global__ __launch_bounds__(64 * (kRingLoaders + 1)) void km_ring_kernel(
    const float* __restrict__ X, int n, int d, PartWs pw, float* __restrict__ out0, float* __restrict__ out1,
    uint64_t active) {
    const int* __restrict__ order = nullptr;
    const int* __restrict__ off = nullptr;
    if constexpr (kMode == 0) {
        const int rs = blockIdx.z;
        if (!((active >> rs) & 1)) return;
        order = pw.order(rs);
        off = pw.off(rs);
        out0 += (int64_t)rs * pw.k * d;
        out1 += (int64_t)rs * pw.k;
    }
    // [slot][column][row]: a lane's 64 rows of its column are contiguous (b128 writes and reads; the 68-float
    // pitch puts 16 consecutive lanes' 16-byte accesses in distinct banks), 139 KB
    __shared__ __align__(16) float ring[kRingSlots][64][kRingPitch];
    __shared__ int ready[kRingSlots];            // chunk held by the slot (-1: none yet)
    __shared__ int done;                         // chunks the adder has consumed
    const int j = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + l;
    const float* __restrict__ Xc = X + (c < d ? c : d - 1);
    const int r0 = kMode == 0 ? off[j] : 0, m = kMode == 0 ? off[j + 1] - r0 : n;
    const int nch = (m + 63) / 64;
    const int total = (kMode == 1 && out1) ? 2 * nch : nch;   // chunk ch covers entries (ch % nch) * 64 + 0..63
    if (threadIdx.x < kRingSlots) ready[threadIdx.x] = -1;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();   // the only block-wide barrier: every wave reaches it before the roles split
    if (w == 0) {
        float acc = 0.f, mean = 0.f;
        for (int ch = 0; ch < total; ++ch) {
            const int s = ch % kRingSlots;
            const bool sq = kMode == 1 && ch >= nch;
            if (kMode == 1 && ch == nch) {   // pass 2 of X.mean / np.var
                mean = acc / (float)m;
                acc = 0.f;
            }
            auto add = [&](float x) {
                if (sq) {
                    const float e = x - mean;
                    acc = __fadd_rn(acc, __fmul_rn(e, e));
                } else {
                    acc += x;
                }
            };
            while (lds_acquire(&ready[s]) != ch) __builtin_amdgcn_s_sleep(1);
            const float4* col = reinterpret_cast<const float4*>(&ring[s][l][0]);
            const int e0 = (ch % nch) * 64;
            if (e0 + 64 <= m) {
                float4 q[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) q[r] = col[r];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    add(q[r].x);
                    add(q[r].y);
                    add(q[r].z);
                    add(q[r].w);
                }
            } else {
                const float* cf = &ring[s][l][0];
                for (int r = 0; r < m - e0; ++r) add(cf[r]);
            }
            if (l == 0) lds_release(&done, ch + 1);
        }
        if (kMode == 0) {
            if (c < d) out0[(int64_t)j * d + c] = acc;
            if (blockIdx.x == 0 && l == 0) out1[j] = (float)m;
        } else if (c < d) {
            if (out1) {
                out0[c] = mean;
                out1[c] = acc / (float)m;
            } else {
                out0[c] = acc / (float)m;
            }
        }
        return;
    }
    // loader w - 1: chunks w - 1, w - 1 + 15, ...; entries past the list end re-read its last row (never added)
    auto row_of = [&](int ch) {
        const int e = min((ch % nch) * 64 + l, m - 1);
        return kMode == 0 ? order[r0 + e] : e;
    };
    int ch = w - 1;
    if (ch >= total) return;
    float v[64];
    int idx = row_of(ch);
#pragma unroll
    for (int t = 0; t < 64; ++t) v[t] = Xc[(int64_t)__builtin_amdgcn_readlane(idx, t) * d];
    for (; ch < total; ch += kRingLoaders) {
        const int nx = ch + kRingLoaders;
        if (nx < total) idx = row_of(nx);
        const int s = ch % kRingSlots;
        while (lds_acquire(&done) < ch - kRingSlots + 1) __builtin_amdgcn_s_sleep(1);   // slot's last chunk added
        float4* col = reinterpret_cast<float4*>(&ring[s][l][0]);
#pragma unroll
        for (int t = 0; t < 16; ++t) col[t] = make_float4(v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]);
        if (l == 0) lds_release(&ready[s], ch);
        if (nx < total) {
#pragma unroll
            for (int t = 0; t < 64; ++t) v[t] = Xc[(int64_t)__builtin_amdgcn_readlane(idx, t) * d];
        }
    }
}

// sklearn _euclidean_dense_dense(squared=True): float32 sum of 4-element groups, then the d % 4 tail
__device__ __forceinline__ float km_euclid_f32(const float* a, const float* b, int d) {
    float r = 0.f;
    const int q = d / 4;
    for (int g = 0; g < q; ++g) {
        const float d0 = a[4 * g] - b[4 * g], d1 = a[4 * g + 1] - b[4 * g + 1];
        const float d2 = a[4 * g + 2] - b[4 * g + 2], d3 = a[4 * g + 3] - b[4 * g + 3];
        r += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    for (int c = 4 * q; c < d; ++c) {
        const float e = a[c] - b[c];
        r += e * e;
    }
    return r;
}
// out[i] = km_euclid_f32(X[i], C[labels[i]]); restart-batched: blockIdx.y = restart (C + r k d, labels / out + r n)
__global__ void km_rowdist_kernel(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ C, int k,
                                  const int32_t* __restrict__ labels, float* __restrict__ out) {
    C += (int64_t)blockIdx.y * k * d;
    labels += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = km_euclid_f32(X + i * d, C + (int64_t)labels[i] * d, d);
}
// float32 sum of v[0..n) in index order: one wave stages 1024 values per round in LDS (coalesced loads,
// the next round prefetched in registers); lane 0 adds them sequentially from LDS.
__global__ __launch_bounds__(64) void km_seqsum_kernel(const float* __restrict__ v, int64_t n, float* out) {
    v += (int64_t)blockIdx.x * n;   // restart-batched: one wave per restart
    out += blockIdx.x;
    __shared__ __align__(16) float buf[64 * kLabQ];
    const int lane = threadIdx.x;
    float cur[kLabQ], nxt[kLabQ];
#pragma unroll
    for (int q = 0; q < kLabQ; ++q) {
        const int64_t i = (int64_t)q * 64 + lane;
        cur[q] = i < n ? v[i] : 0.f;
    }
    float s = 0.f;
    for (int64_t base = 0; base < n; base += 64 * kLabQ) {
        const int64_t nb = base + 64 * kLabQ;
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) {
            const int64_t i = nb + (int64_t)q * 64 + lane;
            nxt[q] = i < n ? v[i] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) buf[q * 64 + lane] = cur[q];
        __syncthreads();
        if (lane == 0) {
            const int m = (int)((n - base) < 64 * kLabQ ? (n - base) : 64 * kLabQ);
            int t = 0;
            // 64 values per batch: 16 b128 reads in flight, then the in-order adds
            for (; t + 64 <= m; t += 64) {
                float4 q[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) q[r] = reinterpret_cast<const float4*>(buf + t)[r];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s += q[r].x;
                    s += q[r].y;
                    s += q[r].z;
                    s += q[r].w;
                }
            }
            for (; t < m; ++t) s += buf[t];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kLabQ; ++q) cur[q] = nxt[q];
    }
    if (lane == 0) out[0] = s;
}

// ---- k-means++ for R restarts in lockstep (cluster.KMeans._kmeans_plusplus_batch; sklearn _kmeans_plusplus)
// Per restart r the previous step's distances prev [R][prevT][n] hold its closest-distance row at trial best[r].
constexpr int kPpMax = 64;      // restarts x trials per launch
struct PpArgs {
    int best[kPpMax];           // per restart: the row of prev holding closest_dist_sq (0 on the first step)
    double rv[kPpMax];          // per (restart, trial): rand_vals = uniform * pot (host: numpy's f64 product)
};
// searchsorted(np.cumsum(closest, dtype=float64), rv) without the sequential cumsum: a parallel prefix S^ of the
// non-negative float64 terms is within B_i = 2 (i + h + 8) 2^-53 S^_i of BOTH the exact prefix and numpy's
// sequential c_i (recursive-summation bounds gamma_i, gamma_h; h = the additions along S^'s evaluation tree), so
//   lo = first i with S^_i + B_i >= rv  and  hi = first i with S^_i - B_i >= rv
// bracket numpy's answer: lo == hi is it exactly; lo != hi (rv within ~1e-11 relative of a prefix, or inside a
// run of zero distances) is flagged and the host redoes that trial with numpy.  cand = min(ans, n - 1) (sklearn's
// clip).  One 1024-thread block per restart: 16 waves x contiguous segments, a lane-strided pass for the segment
// totals, then per 64-element row a wave scan; the first hit per trial and wave is kept with one LDS atomicMin.
__global__ __launch_bounds__(1024) void km_pp_search_kernel(const float* __restrict__ prev, int prevT, int64_t n,
                                                            int T, PpArgs a, int64_t* __restrict__ cand,
                                                            int32_t* __restrict__ amb) {
    const int r = blockIdx.x;
    const float* __restrict__ v = prev + ((int64_t)r * prevT + a.best[r]) * n;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __shared__ double wtot[16], wbase[16];
    __shared__ long long lo[kPpMax], hi[kPpMax];
    const int64_t rows = ((n + 63) / 64 + 15) / 16;            // 64-element rows per wave segment
    const int64_t s0 = (int64_t)w * rows * 64;
    if (threadIdx.x < T) {
        lo[threadIdx.x] = n;
        hi[threadIdx.x] = n;
    }
    double part = 0.0;
    for (int64_t q = 0; q < rows; ++q) {
        const int64_t i = s0 + q * 64 + l;
        part += i < n ? (double)v[i] : 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (l == 0) wtot[w] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int k = 0; k < 16; ++k) {
            wbase[k] = run;
            run += wtot[k];
        }
    }
    __syncthreads();
    const double h = 2.0 * (double)rows + 40.0;
    const double u2 = 2.0 * 0x1p-53;
    double run = wbase[w];
    uint64_t open = (T >= 64 ? ~0ull : ((1ull << T) - 1)) << 0;  // trials whose lo / hi this wave still seeks
    uint64_t open_hi = open;
    for (int64_t q = 0; q < rows && (open | open_hi); ++q) {
        const int64_t i = s0 + q * 64 + l;
        const double x = wave_incl_scan(i < n ? (double)v[i] : 0.0, l);
        const double S = run + x;
        const double B = u2 * ((double)i + h + 8.0) * S;
        for (int t = 0; t < T; ++t) {
            const uint64_t bit = 1ull << t;
            if (open & bit) {
                const uint64_t m = __ballot(i < n && S + B >= a.rv[r * T + t]);
                if (m) {
                    if (l == 0) atomicMin(&lo[t], (long long)(s0 + q * 64 + __builtin_ctzll(m)));
                    open &= ~bit;
                }
            }
            if (open_hi & bit) {
                const uint64_t m = __ballot(i < n && S - B >= a.rv[r * T + t]);
                if (m) {
                    if (l == 0) atomicMin(&hi[t], (long long)(s0 + q * 64 + __builtin_ctzll(m)));
                    open_hi &= ~bit;
                }
            }
        }
        run += __shfl(x, 63, 64);
    }
    __syncthreads();
    if (threadIdx.x < T) {
        const int t = threadIdx.x;
        const long long a0 = lo[t], a1 = hi[t];
        cand[r * T + t] = (a1 < n ? a1 : n - 1);
        amb[r * T + t] = a0 != a1;
    }
}

// out[r][t][i] = min(closest_r[i], float32(max(0, (-2 a.x_i + ||a||^2) + ||x_i||^2))) in float64 with
// a = X[cand[r][t]] (sklearn _euclidean_distances_upcast + np.minimum(closest, dist)); prev == NULL: no minimum
// (the first centre's distances).  Candidate rows (float64) in LDS; 8 candidates per pass over a row.
// CandT: the device array k-means++ draws into (const int64_t*), or up to 16 host-chosen rows by value (CandList:
// km::sqdist_rows, R = 1, prev == NULL) -- one body, so the two give the same bits for the same candidates.
struct CandList {
    int64_t idx[16];
    __device__ int64_t operator[](int t) const { return idx[t]; }
};
template <typename CandT>
__global__ __launch_bounds__(256) void km_pp_dist_kernel(const float* __restrict__ X, int64_t n, int d, int R, int T,
                                                         const CandT cand, const float* __restrict__ prev, int prevT,
                                                         PpArgs a, float* __restrict__ out) {
    extern __shared__ double sh[];  // [RT][d] + norms [RT]
    const int RT = R * T;
    double* A = sh;
    double* An = sh + (int64_t)RT * d;
    for (int i = threadIdx.x; i < RT * d; i += blockDim.x) A[i] = (double)X[cand[i / d] * d + (i % d)];
    __syncthreads();
    for (int t = threadIdx.x; t < RT; t += blockDim.x)
        An[t] = einsum_sq_f64([&](int c) { return A[(int64_t)t * d + c]; }, d);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* xr = X + i * d;
        const double xx = einsum_sq_f64([&](int c) { return (double)xr[c]; }, d);
        for (int t0 = 0; t0 < RT; t0 += 8) {
            double dot[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) dot[t] = 0.0;
            for (int k = 0; k < d; ++k) {
                const double xv = xr[k];
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (t0 + t < RT) dot[t] = fma(A[(int64_t)(t0 + t) * d + k], xv, dot[t]);
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int rt = t0 + t;
                if (rt >= RT) break;
                const double dd = -2.0 * dot[t] + An[rt] + xx;
                float o = fmaxf((float)dd, 0.f);
                if (prev) {
                    const int r = rt / T;
                    o = fminf(prev[((int64_t)r * prevT + a.best[r]) * n + i], o);
                }
                out[(int64_t)rt * n + i] = o;
            }
        }
    }
}

// ---- Lloyd centre update for R restarts (cluster.KMeans._lloyd_batch): C_new[j] = sums[j] * float32(1 / w[j])
// (sklearn's centers_new *= 1 / weight_in_clusters, the reciprocal in double), info[r] = [||C_new[j] - C_old[j]||^2
// in _euclidean_dense_dense float32 order (j < k), empty-cluster flag].  A restart with an empty cluster writes only
// the flag: the host relocates (sklearn _relocate_empty_clusters_dense) and updates that one.
__global__ __launch_bounds__(256) void km_update_kernel(int k, int d, const float* __restrict__ sums,
                                                        const float* __restrict__ w, const float* __restrict__ C_old,
                                                        float* __restrict__ C_new, float* __restrict__ info,
                                                        uint64_t active) {
    const int r = blockIdx.x;
    if (!((active >> r) & 1)) return;
    sums += (int64_t)r * k * d;
    w += (int64_t)r * k;
    C_old += (int64_t)r * k * d;
    C_new += (int64_t)r * k * d;
    info += (int64_t)r * (k + 1);
    __shared__ int empty;
    if (threadIdx.x == 0) empty = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x)
        if (w[j] == 0.f) empty = 1;
    __syncthreads();
    if (empty) {
        if (threadIdx.x == 0) info[k] = 1.f;
        return;
    }
    for (int i = threadIdx.x; i < k * d; i += blockDim.x) {
        const int j = i / d;
        C_new[i] = sums[i] * (float)(1.0 / (double)w[j]);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x)
        info[j] = km_euclid_f32(C_new + (int64_t)j * d, C_old + (int64_t)j * d, d);
    if (threadIdx.x == 0) info[k] = 0.f;
}

}  // namespace

namespace km {

int center(hipStream_t s, const float* X, int64_t n, int d, float* mean, float* var, float* Xc) {
    HLMC_CHECK_ARG(X && mean && Xc && n > 0 && d > 0, "bad km_center arguments");
    HLMC_CHECK_ARG(n < (int64_t)1 << 30, "km_center: n too large");
    km_ring_kernel<1><<<(unsigned)((d + 63) / 64), 64 * (kRingLoaders + 1), 0, s>>>(X, (int)n, d, PartWs{}, mean, var,
                                                                                   1);
    HLMC_LAUNCHED();
    km_sub_kernel<<<(unsigned)std::min<int64_t>(8192, (n * d + 255) / 256), 256, 0, s>>>(X, n, d, mean, Xc);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int sqdist_rows(hipStream_t s, const float* X, int64_t n, int d, const int64_t* cand, int ncand, float* out) {
    HLMC_CHECK_ARG(X && cand && out && ncand >= 1 && ncand <= 16 && d <= 512, "bad km_sqdist_rows arguments");
    HLMC_CHECK_ARG(n > 0 && d > 0, "bad km_sqdist_rows sizes");
    CandList c{};
    for (int t = 0; t < ncand; ++t) {
        HLMC_CHECK_ARG(cand[t] >= 0 && cand[t] < n, "candidate index out of range");
        c.idx[t] = cand[t];
    }
    const size_t sh = ((size_t)ncand * d + ncand) * sizeof(double);
    km_pp_dist_kernel<CandList><<<(unsigned)std::min<int64_t>(4096, (n + 255) / 256), 256, sh, s>>>(
        X, n, d, 1, ncand, c, nullptr, 1, PpArgs{}, out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

static uint64_t mask_of(int R) { return R >= 64 ? ~0ull : ((1ull << R) - 1); }

int assign_batch(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, int R, uint64_t active,
                 int32_t* labels, const int32_t* old, int32_t* n_changed) {
    HLMC_CHECK_ARG(X && C && labels && n > 0 && d > 0 && k > 0 && R >= 1 && R <= 64, "bad km_assign arguments");
    const size_t sh = ((size_t)k * (d + 1) + k + (size_t)kRows * (d + 1)) * sizeof(float);
    HLMC_CHECK_ARG(sh <= 160 * 1024, "k * d too large for LDS");
    km_assign_kernel<<<dim3((unsigned)((n + kRows - 1) / kRows), (unsigned)R), 256, sh, s>>>(X, n, d, C, k, labels, old,
                                                                                           n_changed, active & mask_of(R));
    HLMC_LAUNCHED();
    return HLMC_OK;
}
int assign(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, int32_t* labels, const int32_t* old,
           int32_t* n_changed) {
    return assign_batch(s, X, n, d, C, k, 1, 1, labels, old, n_changed);
}

static int sums_small(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, int R,
                      uint64_t active, float* sm, float* w) {
    km_sums_kernel<<<dim3((unsigned)((d + 63) / 64), (unsigned)k, (unsigned)R), 64, 0, s>>>(X, (int)n, d, labels, k, sm,
                                                                                          w, active);
    HLMC_LAUNCHED();
    return HLMC_OK;
}
int sums(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sm, float* w) {
    HLMC_CHECK_ARG(X && labels && sm && w && k > 0, "bad km_sums arguments");
    HLMC_CHECK_ARG(n > 0 && n < (int64_t)1 << 30 && d > 0 && k <= 65535, "bad km_sums sizes");
    return sums_small(s, X, n, d, labels, k, 1, 1, sm, w);
}

constexpr int64_t kPartMinRows = 4096;
size_t sums_ws(int64_t n, int k) { return layout(n, k).total; }
int sums_batch(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, int R, uint64_t active,
               float* sm, float* w, void* ws, size_t ws_bytes) {
    HLMC_CHECK_ARG(X && labels && sm && w && ws && k > 0 && d > 0 && R >= 1 && R <= 64, "bad km_sums_part arguments");
    HLMC_CHECK_ARG(n > 0 && n < (int64_t)1 << 30 && k <= 8192, "bad km_sums_part sizes");
    const Layout l = layout(n, k);
    HLMC_CHECK_ARG(ws_bytes >= (size_t)R * l.total, "km_sums_part workspace too small");
    active &= mask_of(R);
    if (n <= kPartMinRows) return sums_small(s, X, n, d, labels, k, R, active, sm, w);  // one pass beats four here
    const int tiles = l.tiles;
    PartWs pw{static_cast<char*>(ws), (int64_t)l.total, tiles, k};
    const size_t klds = (size_t)k * sizeof(int);
    int nbits = 0;
    while ((1 << nbits) < k) ++nbits;
    km_part_hist_kernel<<<dim3(tiles, R), 64, klds, s>>>(labels, (int)n, k, nbits, pw, active);
    HLMC_LAUNCHED();
    km_part_scan_kernel<<<R, 1024, klds + sizeof(int), s>>>(pw, active);
    HLMC_LAUNCHED();
    km_part_scatter_kernel<<<dim3(tiles, R), 64, klds, s>>>(labels, (int)n, k, nbits, pw, active);
    HLMC_LAUNCHED();
    km_ring_kernel<0><<<dim3((unsigned)((d + 63) / 64), (unsigned)k, (unsigned)R), 64 * (kRingLoaders + 1), 0, s>>>(
        X, (int)n, d, pw, sm, w, active);
    HLMC_LAUNCHED();
    return HLMC_OK;
}
int sums_part(hipStream_t s, const float* X, int64_t n, int d, const int32_t* labels, int k, float* sm, float* w,
              void* ws, size_t ws_bytes) {
    return sums_batch(s, X, n, d, labels, k, 1, 1, sm, w, ws, ws_bytes);
}

int update_batch(hipStream_t s, int k, int d, int R, uint64_t active, const float* sm, const float* w,
                 const float* C_old, float* C_new, float* info) {
    HLMC_CHECK_ARG(sm && w && C_old && C_new && info && k > 0 && d > 0 && R >= 1 && R <= 64, "bad km_update arguments");
    km_update_kernel<<<R, 256, 0, s>>>(k, d, sm, w, C_old, C_new, info, active & mask_of(R));
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int pp_search(hipStream_t s, int64_t n, int R, int T, const float* prev, int prevT, const int32_t* best,
              const double* rvals, int64_t* cand, int32_t* amb) {
    HLMC_CHECK_ARG(prev && best && rvals && cand && amb && n > 0 && prevT >= 1, "bad km_pp_search arguments");
    HLMC_CHECK_ARG(R >= 1 && T >= 1 && R <= kPpMax && T <= kPpMax && R * T <= kPpMax,
                   "km_pp_search: restarts x trials outside [1, 64]");
    PpArgs a{};
    for (int r = 0; r < R; ++r) {
        HLMC_CHECK_ARG(best[r] >= 0 && best[r] < prevT, "km_pp_search: best row out of range");
        a.best[r] = best[r];
    }
    for (int i = 0; i < R * T; ++i) a.rv[i] = rvals[i];
    km_pp_search_kernel<<<R, 1024, 0, s>>>(prev, prevT, n, T, a, cand, amb);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int pp_dist(hipStream_t s, const float* X, int64_t n, int d, int R, int T, const int64_t* cand, const float* prev,
            int prevT, const int32_t* best, float* out) {
    HLMC_CHECK_ARG(X && cand && out && n > 0 && d > 0, "bad km_pp_dist arguments");
    HLMC_CHECK_ARG(R >= 1 && T >= 1 && R <= kPpMax && T <= kPpMax && R * T <= kPpMax,
                   "km_pp_dist: restarts x trials outside [1, 64]");
    const size_t sh = ((size_t)R * T * d + (size_t)R * T) * sizeof(double);
    HLMC_CHECK_ARG(sh <= 160 * 1024, "km_pp_dist: restarts x trials x d too large for LDS");
    PpArgs a{};
    if (prev) {
        HLMC_CHECK_ARG(best && prevT >= 1, "km_pp_dist: prev needs best rows");
        for (int r = 0; r < R; ++r) {
            HLMC_CHECK_ARG(best[r] >= 0 && best[r] < prevT, "km_pp_dist: best row out of range");
            a.best[r] = best[r];
        }
    }
    km_pp_dist_kernel<const int64_t* __restrict__><<<(unsigned)std::min<int64_t>(4096, (n + 255) / 256), 256, sh, s>>>(
        X, n, d, R, T, cand, prev, prevT, a, out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

int inertia_batch(hipStream_t s, const float* X, int64_t n, int d, const float* C, int k, const int32_t* labels, int R,
                  float* out, float* tmp) {
    HLMC_CHECK_ARG(X && C && labels && out && tmp, "bad km_inertia arguments");
    HLMC_CHECK_ARG(n > 0 && d > 0 && k > 0 && R >= 1 && R <= 64, "bad km_inertia sizes");
    km_rowdist_kernel<<<dim3((unsigned)std::min<int64_t>(4096, (n + 255) / 256), (unsigned)R), 256, 0, s>>>(
        X, n, d, C, k, labels, tmp);
    HLMC_LAUNCHED();
    km_seqsum_kernel<<<R, 64, 0, s>>>(tmp, n, out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}
int inertia(hipStream_t s, const float* X, int64_t n, int d, const float* C, const int32_t* labels, float* out,
            float* tmp) {
    return inertia_batch(s, X, n, d, C, 1, labels, 1, out, tmp);
}

int rowdist(hipStream_t s, const float* X, int64_t n, int d, const float* C, const int32_t* labels, float* out) {
    HLMC_CHECK_ARG(X && C && labels && out, "bad km_rowdist arguments");
    HLMC_CHECK_ARG(n > 0 && d > 0, "bad km_rowdist sizes");
    km_rowdist_kernel<<<(unsigned)std::min<int64_t>(4096, (n + 255) / 256), 256, 0, s>>>(X, n, d, C, 1, labels, out);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

}  // namespace km
}  // namespace hlmc
