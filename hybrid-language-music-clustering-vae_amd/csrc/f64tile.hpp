// The 64 x 64 float64 MFMA tile of dbscan.hip, ward.hip and pca.hip: 256 threads = 4 waves own a
// 64 x 64 output tile and walk the inner (summed) axis in chunks of kKC staged through LDS as doubles.  This header
// owns the format -- the two LDS operand images, which thread stages which element, the lane maps of
// v_mfma_f64_16x16x4_f64 -- and holds loads, float-to-double conversions, the caller's element transform, LDS traffic
// and MFMA calls only: no a * b + c of its own, so it means the same with and without -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace hlmc {
namespace f64tile {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;                  // rows and columns of a block's output tile
constexpr int kKC = 32;                    // inner elements staged per LDS fill
constexpr int kPer = kTile * kKC / 256;    // elements of one image a thread stages per chunk

// Operand images: views over __shared__ doubles the kernel declares (ward_pdist_kernel reuses the storage), stored
// [major][minor] with kMinor elements per line; el(m, k) is tile row (A) or tile column (B) m at inner index k.

// [64][kKC], k contiguous.  An MFMA lane reads (16 w + lr) * kStride + kk + lk: an 8-byte read is served per 32-lane
// half over 32 bank pairs, and 34 lr + lk = 2 lr + lk mod 32 spreads the half's 16 rows x 2 k over all of them.
struct RowImage {
    static constexpr int kMinor = kKC, kStride = kKC + 2, kDoubles = kTile * kStride;
    double* p;
    __device__ __forceinline__ double& at(int major, int minor) const { return p[major * kStride + minor]; }
    __device__ __forceinline__ double& el(int m, int k) const { return at(m, k); }
};

// [kKC][64], the tile's 64 rows or columns contiguous.  A lane reads (kk + lk) * kStride + 16 t + lr; a 32-lane half
// holds lk in {0, 1} (or {2, 3}) x 16 lr, and kStride = 16 mod 32 puts its two k lines on the two halves of the banks.
struct KImage {
    static constexpr int kMinor = kTile, kStride = kTile + 16, kDoubles = kKC * kStride;
    double* p;
    __device__ __forceinline__ double& at(int major, int minor) const { return p[major * kStride + minor]; }
    __device__ __forceinline__ double& el(int m, int k) const { return at(k, m); }
};

// Stager of one image from a row-major matrix of T with leading dimension ld whose lines run the image's way (sample
// rows along k for RowImage; the inner axis down the rows for KImage).  A thread takes minor index tid % kMinor of the
// majors tid / kMinor + kStep u: column tid & 31 of rows (tid >> 5) + 8 u, or column lane of inner rows
// wv + 4 u; a wave reads whole line segments.  fetch() loads the window starting at (major0, minor0) into registers,
// zero past major_end / minor_end; commit() widens to double and stores.  Two steps, so that a kernel can fetch the
// next chunk while the MFMAs of this one run.  commit(img, f) stores f((double)x) for the elements that were inside
// the matrix and 0.0 for the rest: the zero fill is never transformed.
template <class Image, class T>
struct Stage {
    T v[kPer];
    bool in[kPer];
    static __device__ __forceinline__ int minor() { return (int)threadIdx.x % Image::kMinor; }
    static constexpr int kStep = 256 / Image::kMinor;
    static __device__ __forceinline__ int major(int u) { return (int)threadIdx.x / Image::kMinor + kStep * u; }
    __device__ __forceinline__ void fetch(const T* __restrict__ X, int ld, int64_t major0, int64_t major_end,
                                          int minor0, int minor_end) {
        // one per-thread offset plus wave-uniform line steps (scalar registers), not eight 64-bit vector addresses
        const int64_t first = (major0 + major(0)) * ld + minor0 + minor();
        const bool cm = minor0 + minor() < minor_end;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            in[u] = cm && major0 + major(u) < major_end;
            v[u] = in[u] ? X[first + (int64_t)(kStep * u) * ld] : T(0);
        }
    }
    __device__ __forceinline__ void commit(const Image& img) const {
#pragma unroll
        for (int u = 0; u < kPer; ++u) img.at(major(u), minor()) = (double)v[u];
    }
    template <class F>
    __device__ __forceinline__ void commit(const Image& img, F f) const {
#pragma unroll
        for (int u = 0; u < kPer; ++u) img.at(major(u), minor()) = in[u] ? f((double)v[u]) : 0.0;
    }
};

// Inner steps of a chunk with `left` elements to go: all of kKC, or the tail rounded up to the MFMA's 4 (zero-filled)
__device__ __forceinline__ int k_steps(int64_t left) { return (int)min((int64_t)kKC, (left + 3) & ~(int64_t)3); }

// acc += A B over inner indices [0, kmax) of the staged chunk, 4 at a time in ascending order: wave w's rows 16 w ..
// 16 w + 15 against the four 16-column groups.  Operand maps of the f64 MFMA: a lane holds A[row lane & 15][k lane >> 4]
// and B[k lane >> 4][col lane & 15].
template <class ImageA, class ImageB>
__device__ __forceinline__ void mma_chunk(double4_t (&acc)[4], const ImageA& A, const ImageB& B, int kmax) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    for (int kk = 0; kk < kmax; kk += 4) {
        const double a = A.el(wv * 16 + lr, kk + lk);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, B.el(t * 16 + lr, kk + lk), acc[t], 0, 0, 0);
    }
}

// C/D map of the f64 MFMA (col = lane & 15, row = (lane >> 4) + 4 * reg): acc[t][q] is tile row acc_row(q), tile
// column acc_col(t)
__device__ __forceinline__ int acc_row(int q) {
    return (int)(threadIdx.x >> 6) * 16 + (int)((threadIdx.x & 63) >> 4) + 4 * q;
}
__device__ __forceinline__ int acc_col(int t) { return t * 16 + (int)(threadIdx.x & 15); }

}  // namespace f64tile
}  // namespace hlmc
