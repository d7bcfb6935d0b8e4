// Launchers for the MFMA GEMM families (tile choice + deterministic split-K planning).
#include "gemm.hpp"
#include "halo.hpp"
#include "ops.hpp"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace hlmc {
namespace {

// split-K grid targets (A/B on the bench step, scripts in DESIGN.md §8): NT (forward / data-gradient convs,
// linears) 512: 101.8k vs 101.2k at 256 (round 2, after the small split-K grids moved to the LDS-DMA ring;
// round 1 measured 256 ahead of 512 and 128); TN (weight gradients) 192, twice that for K >= kTnLongK (round 1
// measured 512: 93.2k vs 92.8k at 1024, 90.7k at 2048; the later rounds that brought it to 192 are at plan_tn)
constexpr int kNtTargetBlocks = 512;
constexpr int kTnTargetBlocks = 192;
constexpr int kTnLongK = 131072;
constexpr int kTnKch8Min = 1024;
// XCD-aware block order (gemm.hpp xcd_logical_block) for these op kinds: measured per layer (scripts/bench_gemm.py),
// it helps the TN (weight-gradient) family and slows the sub-pixel / conv NT families by 10-20 %
constexpr int kXcdRemapKinds = probe::kWgradS2 | probe::kLinearWgrad;

// Split-K plan: S splits of ksl reduction rows each.
struct Plan {
    int S, ksl;
};
// A tile shape as a type.  Each family names its shapes in one place, with_nt_tile / with_linear_tile / with_tn_tile,
// which calls f with the family's choice for a problem; a launch and its workspace query both go through it and
// through the same nt_plan / tn_plan, so they cannot disagree.
template <int BM_, int BN_, int WM_, int WN_>
struct Tile {
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_;
};
// The grid of a launch under one tile shape: M x N tiles (per phase), the split-K plan, the bytes of its fp32 slabs
struct GemmPlan {
    int tiles;
    Plan pl;
    size_t slab_bytes;
};
// BK = the largest K-step (split ranges are multiples of it); the minimum work per split is counted in
// steps of the short (BK/2) K-step the kernel uses for short ranges
inline Plan plan_nt(int tiles, int Kmax, int BK) {
    constexpr int target = kNtTargetBlocks;
    int S = 1;
    if (tiles < target / 2) {
        S = cdiv(target, tiles);
        S = std::min(S, std::max(1, Kmax / (2 * BK)));
    }
    int ksl = cdiv(cdiv(Kmax, S), BK) * BK;
    S = cdiv(Kmax, ksl);
    return {S, ksl};
}
inline Plan plan_tn(int tiles, int K, int BK) {
    // weight gradients: long K (= batch x pixels), tiny M x N: split K until the grid fills the chip
    // (>= 4 k-tiles per split); the slab reduction keeps 4 loads in flight.  The longest reductions (the
    // 32 / 64-channel layers, K = 262 144) take a 1024-block grid: per layer (scripts/gpu_wgrad_blocks.sh,
    // bench_gemm.py) 47 vs 60 us at 512, while every shorter layer is fastest at 512 (1024: +10-20 %).
    // Round 4 (with the NT GEMMs at two blocks per CU beside them): one 256-block target for every layer measured
    // 134.1k vs 132.9k clips/s at 512 / 1024 (128: 129.6k, 192: 133.6k, 320: 133.6k, 384: 132.1k, 768: 130.8k);
    // the long layers at 512 then 134.5k vs 134.0k (1024: 134.1k).  Round 6, with the cheap power-of-two loaders: 192
    // 142.5k vs 141.8k at 256, 384 139.2k vs 141.9k (3 pairs each; 384 is 7 % faster standalone: the side-stream grids
    // take CUs from the main stream).
    const int target = K >= kTnLongK ? 2 * kTnTargetBlocks : kTnTargetBlocks;
    int S = cdiv(target, tiles);
    S = std::max(1, std::min(S, K / (4 * BK)));
    int ksl = cdiv(cdiv(K, S), BK) * BK;
    S = cdiv(K, ksl);
    return {S, ksl};
}

// NT pipeline: 0 register-staged (gemm_nt_kernel), 2 = the 2-stage LDS-DMA ring (gemm_nt_glds_kernel).
// Measured (scripts/bench_gemm.py): the DMA ring wins when a block reduces >= 1024 (16 K-steps), the register path
// below that (short reductions: more co-resident blocks hide the pipeline prologue) -- except on split-K grids of
// <= 512 blocks, where the ring wins even on 9-step reductions (the 4x4x512 conv / its data gradient: 21.5 vs
// 31.8 us).  The ring's depth: 2 stages (64 KB of LDS, 176 VGPRs: two blocks per CU, each one K-step ahead)
// measured 131.9k vs 129.3k clips/s with 4 stages (128 KB, one block per CU, three K-steps ahead) and 129.7k with 3;
// split grids on the ring up to 1024 blocks 132.0k (3 rounds each; round 4).
constexpr int kGldsSplitMax = 512;
inline int nt_pipe_select(int ksl, int S, int blocks) {
    if (S > 1 && blocks <= kGldsSplitMax) return 2;
    return ksl >= 1024 ? 2 : 0;
}

inline int xcd_remap_for_site() { return (kXcdRemapKinds & probe::g_site.kind) ? 1 : 0; }

// Register-path launches with 4 sub-pixel phases and >= kPloopTiles M x N tiles (>= 4 blocks per CU without
// the phases) run the phases inside each block (gemm_nt_kernel ploop): the 64 x 64 / 32 x 32 layers' phases
// otherwise stream the low-res input from HBM once per phase (measured round 2: 105.2k vs 104.25k clips/s without,
// both the forward and the data-gradient launches gain).
constexpr int kPloopTiles = 1024;
inline bool use_ploop(int phases, int tmn, int pipe) { return phases >= 2 && pipe == 0 && tmn >= kPloopTiles; }

// TR: transposed accumulators + 4-column vector stores (epilogue_tile_t; needs N % 4 == 0 and 4-aligned row
// strides: the conv / sub-pixel NHWC outputs and their split-K slabs), else the per-element epilogue (linears)
template <typename T, class TL, bool TR, class AL, class BL, class E>
void nt_kernel_launch_tr(hipStream_t s, dim3 grid, const AL& al, const BL& bl, const E& ep, int M, int N, int ksl,
                         bool long_k, int pipe) {
    constexpr int BM = TL::BM, BN = TL::BN, WM = TL::WM, WN = TL::WN;
    const int rm = xcd_remap_for_site();
    const int ploop = use_ploop((int)grid.y, (int)grid.x, pipe) ? (int)grid.y : 1;
    if (ploop > 1) grid.y = 1;
    HLMC_PROBE_BEGIN(s);
    if (pipe == 2)
        gemm_nt_glds_kernel<T, BM, BN, WM, WN, 2, AL, BL, E, TR, 2><<<grid, 256, 0, s>>>(al, bl, ep, M, N, ksl, rm);
    else if (long_k)
        gemm_nt_kernel<T, BM, BN, WM, WN, 8, AL, BL, E, TR><<<grid, 256, 0, s>>>(al, bl, ep, M, N, ksl, rm, ploop);
    else
        gemm_nt_kernel<T, BM, BN, WM, WN, 4, AL, BL, E, TR><<<grid, 256, 0, s>>>(al, bl, ep, M, N, ksl, rm, ploop);
    HLMC_PROBE_END(s);
}
// The transposed-accumulator epilogue for the conv families (N % 4 == 0).  Measured per layer (scripts/bench_gemm.py,
// round 3): it takes the split-K / LDS-DMA conv and sub-pixel GEMMs from 28-42 to 22-32 us (the 8 x 8 .. 2 x 2
// layers), but makes the LDS halo-tile kernels 4-15 % slower (their stores were not the bound; the swapped fragments
// cost LDS issue) -> halo kernels keep the per-element epilogue.

template <typename T, class TL>
GemmPlan nt_plan(int M, int N, int Kmax, int phases) {
    const int tmn = cdiv(M, TL::BM) * cdiv(N, TL::BN);
    const Plan pl = plan_nt(tmn * phases, Kmax, gemm_bk<T>());
    return {tmn, pl, (size_t)phases * pl.S * M * N * sizeof(float)};
}
// register path: short reductions keep the 4-chunk K-step (more co-resident blocks), long ones 8 chunks
inline bool nt_long_k(int Kmax) { return Kmax >= 1024; }

// The GEMM to the plan's fp32 partial slabs alone (S = 1: one slab); a reduce launch follows.
template <typename T, class TL, bool TR, class AL, class BL>
int nt_partials(hipStream_t s, const AL& al, const BL& bl, const GemmPlan& gp, int M, int N, int Kmax, int phases, Ws ws,
                int pipe) {
    HLMC_CHECK_ARG(ws.p && ws.bytes >= gp.slab_bytes, "split-K workspace too small");
    StorePartialZ part;
    part.ws = ws.p; part.M = M; part.N = N; part.S = gp.pl.S; part.phase = 0; part.split = 0;
    nt_kernel_launch_tr<T, TL, TR>(s, dim3(gp.tiles, phases, gp.pl.S), al, bl, part, M, N, gp.pl.ksl, nt_long_k(Kmax),
                                   pipe);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

template <typename T, class TL, bool TR, class AL, class BL, class EP>
int launch_nt(hipStream_t s, const AL& al, const BL& bl, const EP& ep, int M, int N, int Kmax, int phases, Ws ws,
              ops::ColStats* st = nullptr, bool dma_ok = true) {
    const GemmPlan gp = nt_plan<T, TL>(M, N, Kmax, phases);
    const int S = gp.pl.S, ksl = gp.pl.ksl;
    const int pipe = (dma_ok && TL::BN >= 32 && TL::BM >= 64) ? nt_pipe_select(ksl, S, gp.tiles * phases * S) : 0;
    const bool stats = st && st->acc.on();
    if (st) st->done = false;
    if (S == 1) {  // single pass; with statistics the epilogue also emits the column statistics
        const dim3 grid(gp.tiles, phases, 1);
        const bool long_k = nt_long_k(Kmax);
        if (stats) nt_kernel_launch_tr<T, TL, TR>(s, grid, al, bl, with_stats(ep, st->acc), M, N, ksl, long_k, pipe);
        else nt_kernel_launch_tr<T, TL, TR>(s, grid, al, bl, ep, M, N, ksl, long_k, pipe);
        HLMC_LAUNCHED();
        if (stats) st->done = true;
        return HLMC_OK;
    }
    const int rc = nt_partials<T, TL, TR>(s, al, bl, gp, M, N, Kmax, phases, ws, pipe);
    if (rc != HLMC_OK) return rc;
    const bool idx32 = (double)phases * S * M * N < 2147483648.0;  // 32-bit slab offsets
    if (stats && N % 64 == 0 && idx32) {  // the reduce delivers them
        const int rows = phases * M, ntc = N / 64;
        // the tallest tile (fewest accumulator adds) that still gives >= 1024 blocks (A/B: 128 / 256 / 512 / 1024)
        const int RU = cdiv(rows, 128) * ntc >= 1024 ? 32 : cdiv(rows, 64) * ntc >= 1024 ? 16 : 8;
        const unsigned nb = (unsigned)(cdiv(rows, 4 * RU) * ntc);
        switch (RU) {
            case 32: splitk_reduce_stats_kernel<EP, 32><<<nb, 256, 0, s>>>(ws.p, ep, M, N, S, phases, st->acc); break;
            case 16: splitk_reduce_stats_kernel<EP, 16><<<nb, 256, 0, s>>>(ws.p, ep, M, N, S, phases, st->acc); break;
            default: splitk_reduce_stats_kernel<EP, 8><<<nb, 256, 0, s>>>(ws.p, ep, M, N, S, phases, st->acc); break;
        }
        HLMC_LAUNCHED();
        st->done = true;
        return HLMC_OK;
    }
    const int64_t total = (int64_t)phases * M * N;
    const FastDiv dN((uint32_t)N), dM((uint32_t)M);
    if (N % 4 == 0 && idx32 && ((uintptr_t)ws.p & 15) == 0) {
        const unsigned nb = (unsigned)((total / 4 + 255) / 256);
        splitk_reduce_kernel<4, EP><<<nb, 256, 0, s>>>(ws.p, ep, M, N, S, phases, dN, dM);
    } else {
        const int blocks = (int)std::min<int64_t>(4096, (total + 255) / 256);
        splitk_reduce_kernel<1, EP><<<blocks, 256, 0, s>>>(ws.p, ep, M, N, S, phases, dN, dM);
    }
    HLMC_LAUNCHED();
    return HLMC_OK;
}

// Tile choice for the NT family by N: 128x128 / 128x64 / 128x32.  (Measured: stepping down to 64x64 to put
// two blocks on every CU doubles operand re-reads and is slower on every layer of the step.)
template <class F>
auto with_nt_tile(int M, int N, int phases, F&& f) {
    // 128 x 64 tiles where 128 x 128 tiles would give an unsplit grid of target/2 .. target blocks (one block per
    // CU where two fit: the 2-stage ring and the register path hold two): twice the blocks, no split-K slabs.
    // Measured: 133.1k vs 132.3k clips/s (3 rounds); also for target/4 .. target/2 (then split-K) 131.3k.
    const int t = cdiv(M, 128) * cdiv(N, 128) * phases;
    if (N >= 128 && !(t >= kNtTargetBlocks / 2 && t < kNtTargetBlocks)) return f(Tile<128, 128, 64, 64>{});
    if (N > 32) return f(Tile<128, 64, 32, 64>{});
    return f(Tile<128, 32, 32, 32>{});
}
template <typename T, class AL, class BL, class EP>
int dispatch_nt(hipStream_t s, const AL& al, const BL& bl, const EP& ep, int M, int N, int Kmax, int phases, Ws ws,
                ops::ColStats* st = nullptr) {
    return with_nt_tile(M, N, phases, [&](auto tl) {
        using TL = decltype(tl);
        // conv / sub-pixel outputs are NHWC rows of N (a multiple of 8) channels: transposed-accumulator epilogue
        if (N % 4 == 0) return launch_nt<T, TL, true>(s, al, bl, ep, M, N, Kmax, phases, ws, st);
        return launch_nt<T, TL, false>(s, al, bl, ep, M, N, Kmax, phases, ws, st);
    });
}
// workspace of a split launch: its slabs (none for S = 1)
inline size_t split_ws(const GemmPlan& gp) { return gp.pl.S == 1 ? 0 : gp.slab_bytes; }
template <typename T>
size_t dispatch_nt_ws(int M, int N, int Kmax, int phases) {
    return with_nt_tile(M, N, phases, [&](auto tl) { return split_ws(nt_plan<T, decltype(tl)>(M, N, Kmax, phases)); });
}

// Linear layers have small M (= batch): 64x64 tiles so more blocks exist before split-K.  Register path, per-element
// epilogue: arbitrary ld / K (the DMA path needs 16-byte chunks that never straddle K).
template <class F>
auto with_linear_tile(int M, int N, F&& f) {
    if (M >= 1024 && N >= 128) return f(Tile<128, 128, 64, 64>{});
    return f(Tile<64, 64, 32, 32>{});
}
template <typename T, class AL, class BL, class EP>
int dispatch_linear(hipStream_t s, const AL& al, const BL& bl, const EP& ep, int M, int N, int K, Ws ws) {
    return with_linear_tile(M, N, [&](auto tl) {
        return launch_nt<T, decltype(tl), false>(s, al, bl, ep, M, N, K, 1, ws, nullptr, false);
    });
}
template <typename T>
size_t dispatch_linear_ws(int M, int N, int K) {
    return with_linear_tile(M, N, [&](auto tl) { return split_ws(nt_plan<T, decltype(tl)>(M, N, K, 1)); });
}
// dispatch_linear's GEMM to the partial slabs alone; the caller reduces the *S_out slabs.
template <typename T, class AL, class BL>
int dispatch_linear_partials(hipStream_t s, const AL& al, const BL& bl, int M, int N, int K, Ws ws, int* S_out) {
    return with_linear_tile(M, N, [&](auto tl) {
        const GemmPlan gp = nt_plan<T, decltype(tl)>(M, N, K, 1);
        *S_out = gp.pl.S;
        return nt_partials<T, decltype(tl), false>(s, al, bl, gp, M, N, K, 1, ws, 0);
    });
}

// Final epilogue of a conv weight gradient: C[m][n = tap*C + ci] -> dW[m][ci][tap] (torch layout).
struct StoreWgradConv {
    float* dW;
    int C;
    // the layer's bias gradient (column totals of its exact accumulator) written by the reduce launch's first block
    // (splitk_reduce_grouped_kernel: ep_extra) instead of a separate launch on the weight-gradient stream
    XAcc bacc;
    float* gb = nullptr;
    __device__ void extra() const {
        if (gb && blockIdx.x == 0)
            for (int c = threadIdx.x; c < bacc.ncols; c += blockDim.x) gb[c] = (float)xacc_column(bacc, c);
    }
    struct Row {
        float* r;
    };
    __device__ void set_phase(int) {}
    __device__ Row row(int m) const { return Row{dW + (int64_t)m * C * 9}; }
    __device__ void store(const Row& rw, int n, float v) const {
        int tap = n / C, ci = n - tap * C;
        rw.r[ci * 9 + tap] = v;
    }
};

// Split-K reduction of a conv weight gradient into torch's [M][C][3][3] layout for few splits (S <= 4: the deep
// layers, whose 2-9 MB outputs dominate): one 288-thread block per (row m, 32 VW input channels); thread (tap, cl) sums
// VW consecutive channels of its tap in split order (slab_sum: the same bits at either width; the slab reads: 9 runs
// of 32 VW consecutive floats) and the block writes its 288 VW consecutive dW floats through LDS.
// (splitk_reduce_grouped_kernel stores dW[m][ci][tap] from the GEMM's (tap, ci) column order: stride-9 scattered
// 4-byte stores, 10-13 us for these layers.)  VW 4 (C % 128 == 0, 16-byte aligned ws and dW): 16-byte slab loads and
// dW stores.  (Four-byte loads left too few bytes in flight: 2.6-3.5 TB/s on the 2- and 4-split layers.)
template <int VW>
__global__ __launch_bounds__(288) void splitk_reduce_wgrad_conv_kernel(const float* __restrict__ ws, StoreWgradConv ep,
                                                                       int M, int C, int S) {
    ep_extra(ep, 0);
    constexpr int CB = 32 * VW;  // input channels per block
    __shared__ __attribute__((aligned(16))) float tile[CB * 9];
    const int cb = C / CB;
    const int m = blockIdx.x / cb, ci0 = (blockIdx.x - m * cb) * CB;
    const int t = threadIdx.x, tap = t >> 5, cl = t & 31;
    const int64_t N = 9LL * C, st = (int64_t)M * N;
    const slab_t<VW> acc = slab_sum<VW, 1>(ws + (int64_t)m * N + tap * C + ci0 + VW * cl, st, S, 0);
#pragma unroll
    for (int i = 0; i < VW; ++i) tile[(VW * cl + i) * 9 + tap] = slab_at(acc, i);
    __syncthreads();
    using V = slab_t<VW>;
    *reinterpret_cast<V*>(ep.dW + (int64_t)m * N + (int64_t)ci0 * 9 + VW * t) =
        *reinterpret_cast<const V*>(&tile[VW * t]);
}

// S-way split-K reduction with the splits spread over G thread groups (splitk_reduce_grouped_kernel)
template <class EP>
void reduce_splits(hipStream_t s, const float* ws, const EP& ep, int M, int N, int S) {
    if constexpr (std::is_same<EP, StoreWgradConv>::value) {
        if (S <= 4 && ep.C % 128 == 0 && (((uintptr_t)ws | (uintptr_t)ep.dW) & 15) == 0) {
            splitk_reduce_wgrad_conv_kernel<4><<<(unsigned)(M * (ep.C / 128)), 288, 0, s>>>(ws, ep, M, ep.C, S);
            return;
        }
        if (S <= 4 && ep.C % 32 == 0) {
            splitk_reduce_wgrad_conv_kernel<1><<<(unsigned)(M * (ep.C / 32)), 288, 0, s>>>(ws, ep, M, ep.C, S);
            return;
        }
    }
    const int64_t total = (int64_t)M * N;
    const bool v4 = N % 4 == 0 && ((uintptr_t)ws & 15) == 0;
    auto go = [&](auto gtag) {
        constexpr int G = decltype(gtag)::value;
        const int64_t per = v4 ? 4 * (256 / G) : 256 / G;  // outputs per block
        const int64_t blocks = (total + per - 1) / per;
        if (v4) splitk_reduce_grouped_kernel<4, G, EP><<<(unsigned)blocks, 256, 0, s>>>(ws, ep, M, N, S);
        else splitk_reduce_grouped_kernel<1, G, EP><<<(unsigned)blocks, 256, 0, s>>>(ws, ep, M, N, S);
    };
    if (S >= 32) go(std::integral_constant<int, 8>{});
    else if (S >= 8) go(std::integral_constant<int, 4>{});
    else if (S >= 4) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
}

template <typename T, class TL>
GemmPlan tn_plan(int M, int N, int K) {
    const int tiles = cdiv(M, TL::BM) * cdiv(N, TL::BN);
    const Plan pl = plan_tn(tiles, K, gemm_bk<T>());
    return {tiles, pl, (size_t)pl.S * M * N * sizeof(float)};
}
template <typename T, class TL, class LL, class HL, class EP>
int launch_tn(hipStream_t s, const LL& ll, const HL& hl, const EP& ep, int M, int N, int K, Ws ws) {
    constexpr int BM = TL::BM, BN = TL::BN, WM = TL::WM, WN = TL::WN;
    const GemmPlan gp = tn_plan<T, TL>(M, N, K);
    const Plan pl = gp.pl;
    HLMC_CHECK_ARG(ws.p && ws.bytes >= gp.slab_bytes, "wgrad workspace too small");
    dim3 grid(gp.tiles, 1, pl.S);
    const int rm = xcd_remap_for_site();
    HLMC_PROBE_BEGIN(s);
    // the 64-deep K-step for splits of >= 1024 rows (measured: 490.9 vs 450.9 us for the 9 conv layers when
    // every split took it), the 32-deep one below; branch-free 16-byte loads where both operands allow them
    const bool vec = ll.vec_ok() && hl.vec_ok();
    constexpr int NTH = 64 * (BM / WM) * (BN / WN);
    auto go = [&](auto out) {
        using OUT = decltype(out);
        if (pl.ksl >= kTnKch8Min) {
            if (vec) gemm_tn_kernel<T, BM, BN, WM, WN, 8, LL, HL, true, OUT><<<grid, NTH, 0, s>>>(ll, hl, out, M, N, K, pl.ksl, rm);
            else gemm_tn_kernel<T, BM, BN, WM, WN, 8, LL, HL, false, OUT><<<grid, NTH, 0, s>>>(ll, hl, out, M, N, K, pl.ksl, rm);
        } else {
            if (vec) gemm_tn_kernel<T, BM, BN, WM, WN, 4, LL, HL, true, OUT><<<grid, NTH, 0, s>>>(ll, hl, out, M, N, K, pl.ksl, rm);
            else gemm_tn_kernel<T, BM, BN, WM, WN, 4, LL, HL, false, OUT><<<grid, NTH, 0, s>>>(ll, hl, out, M, N, K, pl.ksl, rm);
        }
    };
    if constexpr (tn_direct<EP>::value) {
        if (pl.S == 1) {  // one split (the dense layers' batch-long reductions): the epilogue stores from registers
            go(TnDirect<EP>{ep});
            HLMC_PROBE_END(s);
            HLMC_LAUNCHED();
            return HLMC_OK;
        }
    }
    go(TnSlab{ws.p});
    HLMC_PROBE_END(s);
    HLMC_LAUNCHED();
    reduce_splits(s, ws.p, ep, M, N, pl.S);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

// Weight-gradient tile choice.  Weight gradients reduce over K = B * pixels (16 k - 262 k) into a small
// M x N output; the grid is filled by split-K.  Conv weight gradients have N = 9 C: C = 32 gives N = 288,
// which 128-wide tiles cover with 25 % zero columns; 96-wide tiles cover it exactly (measured: 83 -> 72 us for
// the 64 x 288 x 262144 layers).  (Measured and rejected: 64 x 64 tiles everywhere, which cut the split-K slab
// bytes 3-4x but were 10-35 % slower per layer — the kernel is bound by per-block load latency, not slabs.)
inline bool tn_n96(int N) { return N % 128 != 0 && N % 96 == 0; }
template <class F>
auto with_tn_tile(int M, int N, F&& f) {
    if (M >= 128) return f(Tile<128, 128, 64, 64>{});
    if (M > 32) return tn_n96(N) ? f(Tile<64, 96, 32, 48>{}) : f(Tile<64, 128, 32, 64>{});
    return f(Tile<32, 128, 32, 32>{});
}
template <typename T, class LL, class HL, class EP>
int dispatch_tn(hipStream_t s, const LL& ll, const HL& hl, const EP& ep, int M, int N, int K, Ws ws) {
    return with_tn_tile(M, N, [&](auto tl) { return launch_tn<T, decltype(tl)>(s, ll, hl, ep, M, N, K, ws); });
}
template <typename T>
size_t dispatch_tn_ws(int M, int N, int K) {  // slabs at every split count (only a direct epilogue skips S = 1's)
    return with_tn_tile(M, N, [&](auto tl) { return tn_plan<T, decltype(tl)>(M, N, K).slab_bytes; });
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int log2_exact(int c) { return (c > 0 && (c & (c - 1)) == 0) ? __builtin_ctz(c) : -1; }

// ---- the LDS halo-tile kernels (halo.hpp) and their four shapes (bf16).  A row: the shape (Hi a multiple of hdiv:
// whole tiles per image), the tile's pixels (GEMM rows: output pixels of the conv, low-res pixels of the sub-pixel
// conv), and per form the channel splits (blocks per tile) and the grid cap, with the kernels built for them.  The
// statistics and input-BatchNorm forms share a tiling; the plain form (data gradients, eval) may differ.
struct HaloGrid {
    int nspl, cap;
};
template <class EP>
struct HaloShape {
    using Plain = void (*)(const bf16*, int, int, const bf16*, EP, int, ops::BnInput);
    using Stats = void (*)(const bf16*, int, int, const bf16*, WithStats<EP>, int, ops::BnInput);
    int Ci, Co, Wi, hdiv, tp;
    HaloGrid stat, plain;
    Plain k_plain;
    Stats k_stats, k_xin;
};
template <class G, class EP, int WPE, class GP = G, int WPE_P = WPE>  // GP / WPE_P: the plain form's, where it differs
constexpr HaloShape<EP> halo_shape(int hdiv, int cap, int cap_p) {
    return {G::CI, G::CO, G::WI, hdiv, G::TP, {G::NSPL, cap}, {GP::NSPL, cap_p}, halo_kernel<GP, EP, false, WPE_P>,
            halo_kernel<G, WithStats<EP>, false, WPE>, halo_kernel<G, WithStats<EP>, true, WPE>};
}
using ConvEp = StoreRM<bf16>;
using SubEp = StoreSubpixel<bf16>;
// Two blocks per CU (WPE 2, a 512-block grid) where a block fits in half the LDS (<= 80 KB) and 256 VGPRs: the
// co-resident block covers the single halo buffer's extra barrier.
// conv 32 -> 64, Wi 64: 2-row (64-pixel) tiles: 64 KB (73 KB with the input BatchNorm).  Measured in
// the step: forward with the input BatchNorm + statistics 49.6 -> 42.7 us, the decoder data gradient 32.2 -> 31.5 us
// (4-row tiles, two halo buffers, one block per CU before); the same with 4-row tiles and two 32-channel blocks per
// tile (the halo read twice) lost (50 -> 55 / 32 -> 36 us).
// conv 64 -> 128, Wi 32: two 64-channel halves per 64-pixel tile (the weights take half the LDS), one block per CU.
constexpr HaloShape<ConvEp> kConvHalo[] = {
    halo_shape<ConvS2Halo<32, 64, 1, 32, 2>, ConvEp, 2>(8, 512, 512),
    halo_shape<ConvS2Halo<64, 64, 2, 16, 4>, ConvEp, 1>(8, 256, 256),
};
// sub-pixel 64 -> 32, Wi 32, all three forms two per CU: 129.3k vs 128.0k clips/s, 3 alternating rounds (forward
// 53 -> 46 us, data gradient 72 -> 56 us in the step).
// sub-pixel 128 -> 64, Wi 16: the plain form (data gradient) with 16 channels per block (four blocks per tile,
// 79 KB) two per CU 38 -> 33 us, while its statistics / input-BN forms would need 90 KB (one block per CU) and lost
// 48 -> 68 us: they keep 32 channels per block.
constexpr HaloShape<SubEp> kSubpixelHalo[] = {
    halo_shape<SubpixelHalo<64, 32, 1, 32, 4>, SubEp, 2>(4, 512, 512),
    halo_shape<SubpixelHalo<128, 32, 2, 16, 8>, SubEp, 1, SubpixelHalo<128, 16, 4, 16, 8>, 2>(8, 256, 512),
};
template <class EP, size_t N>
const HaloShape<EP>* halo_find(const HaloShape<EP> (&tab)[N], int Ci, int Co, int Wi, int Hi) {
    for (const HaloShape<EP>& h : tab)
        if (h.Ci == Ci && h.Co == Co && h.Wi == Wi && Hi % h.hdiv == 0) return &h;
    return nullptr;
}
// One launch over the M / tp tiles (whole rows: tiles stay inside an image): the statistics form (with the input
// BatchNorm when xin is given) when st has an accumulator, which it then marks delivered, else the plain form.
template <class EP>
int halo_launch(hipStream_t s, const HaloShape<EP>& h, const bf16* x, int Hi, const bf16* wp, const EP& ep, int M,
                ops::ColStats* st, const ops::BnInput* xin) {
    const int ntiles = M / h.tp;
    const bool stats = st && st->acc.on();
    const HaloGrid g = stats ? h.stat : h.plain;
    const int grid = std::min(ntiles * g.nspl, g.cap);
    HLMC_PROBE_BEGIN(s);
    if (stats) {
        (xin ? h.k_xin : h.k_stats)<<<grid, 256, 0, s>>>(x, Hi, ntiles, wp, with_stats(ep, st->acc), M,
                                                         xin ? *xin : ops::BnInput{});
    } else {
        h.k_plain<<<grid, 256, 0, s>>>(x, Hi, ntiles, wp, ep, M, ops::BnInput{});
    }
    if (st) st->done = stats;
    HLMC_PROBE_END(s);
    HLMC_LAUNCHED();
    return HLMC_OK;
}

}  // namespace

namespace ops {

template <typename T>
bool conv_s2_takes_input_bn(int B, int Hi, int Wi, int Ci, int Co) {
    (void)B;
    return std::is_same<T, bf16>::value && halo_find(kConvHalo, Ci, Co, Wi, Hi);
}
template <typename T>
bool subpixel_takes_input_bn(int B, int Hi, int Wi, int Ci, int Co) {
    (void)B;
    return std::is_same<T, bf16>::value && halo_find(kSubpixelHalo, Ci, Co, Wi, Hi);
}

template <typename T>
int conv_s2(hipStream_t s, const T* x, int B, int Hi, int Wi, int Ci, const T* wp, const float* bias, int Co, T* y, Ws ws,
            ColStats* st, const BnInput* xin, const FlatOut* fo) {
    HLMC_CHECK_ARG(!xin || conv_s2_takes_input_bn<T>(B, Hi, Wi, Ci, Co), "conv_s2: input BatchNorm needs a halo shape");
    HLMC_CHECK_ARG(!fo || (!st && !xin), "conv_s2: a flat output with fused statistics / input BatchNorm");
    if (xin) HLMC_CHECK_ARG(xin->acc.p && xin->acc.ncols == 2 * Ci && xin->a_out && st && st->acc.on(),
                            "conv_s2: input BatchNorm arguments");
    constexpr int V = Vec16<T>::N;
    HLMC_CHECK_ARG(Hi % 2 == 0 && Wi % 2 == 0 && Ci % V == 0, "conv_s2: need even H/W and Ci % 8 (bf16) / 4 (f32)");
    HLMC_CHECK_ARG(aligned16(x) && aligned16(wp), "conv_s2: 16-byte alignment");
    const int Ho = Hi / 2, Wo = Wi / 2, M = B * Ho * Wo, K = 9 * Ci;
    ConvS2Loader<T> al{x, Hi, Wi, Ci, Ho, Wo, M, log2_exact(Ci), FastDiv((uint32_t)Wo), FastDiv((uint32_t)Ho)};
    DenseLoader<T> bl{wp, K, Co, K, true};
    StoreRM<T> ep{y, bias, Co, 0, 0};
    probe::site(probe::kConvS2, 2.0 * M * Co * K,
                (double)sizeof(T) * ((double)B * Hi * Wi * Ci + (double)Co * K + (double)M * Co));
    if (fo) {  // NCHW-flat rows for the dense layer that reads the map (the decoder's first layer's data gradient)
        HLMC_CHECK_ARG(fo->ld >= Co * Ho * Wo, "conv_s2: flat row stride");
        StoreNhwcAsFlat<T> ef;
        static_cast<StoreRM<T>&>(ef) = ep;
        ef.relu_ref = static_cast<const T*>(fo->relu_ref);
        ef.fx = FlatIdx(Ho * Wo, Co, fo->ld);
        return dispatch_nt<T>(s, al, bl, ef, M, Co, K, 1, ws, nullptr);
    }
    if constexpr (std::is_same<T, bf16>::value) {
        if (const auto* h = halo_find(kConvHalo, Ci, Co, Wi, Hi)) return halo_launch(s, *h, x, Hi, wp, ep, M, st, xin);
    }
    return dispatch_nt<T>(s, al, bl, ep, M, Co, K, 1, ws, st);
}

template <typename T>
size_t conv_s2_ws(int B, int Hi, int Wi, int Ci, int Co) {
    return dispatch_nt_ws<T>(B * (Hi / 2) * (Wi / 2), Co, 9 * Ci, 1);
}

template <typename T>
int subpixel(hipStream_t s, const T* x, int B, int Hi, int Wi, int Ci, const T* wp, const float* bias, int Co, T* y, Ws ws,
             ColStats* st, const BnInput* xin) {
    HLMC_CHECK_ARG(!xin || subpixel_takes_input_bn<T>(B, Hi, Wi, Ci, Co), "subpixel: input BatchNorm needs a halo shape");
    if (xin) HLMC_CHECK_ARG(xin->acc.p && xin->acc.ncols == 2 * Ci && xin->a_out && st && st->acc.on(),
                            "subpixel: input BatchNorm arguments");
    constexpr int V = Vec16<T>::N;
    HLMC_CHECK_ARG(Ci % V == 0, "subpixel: Ci % 8 (bf16) / 4 (f32)");
    HLMC_CHECK_ARG(aligned16(x) && aligned16(wp), "subpixel: 16-byte alignment");
    const int M = B * Hi * Wi;
    SubpixelLoader<T> al{x, Hi, Wi, Ci, M, log2_exact(Ci), 0, 0, 0, 0, FastDiv((uint32_t)Wi), FastDiv((uint32_t)Hi)};
    SubpixelWeight<T> bl{wp, Ci, Co, log2_exact(Ci), 0, 0, 0, 0};
    StoreSubpixel<T> ep{y, bias, Hi, Wi, Co, 0, 0, FastDiv((uint32_t)Wi), FastDiv((uint32_t)Hi)};
    // the 4 phases hold 1 + 2 + 2 + 4 = 9 taps: 9 Ci MACs per (low-res pixel, output channel)
    probe::site(probe::kSubpixel, 2.0 * M * Co * 9.0 * Ci,
                (double)sizeof(T) * ((double)M * Ci + 9.0 * Ci * Co + 4.0 * M * Co));
    if constexpr (std::is_same<T, bf16>::value) {
        if (const auto* h = halo_find(kSubpixelHalo, Ci, Co, Wi, Hi)) return halo_launch(s, *h, x, Hi, wp, ep, M, st, xin);
    }
    return dispatch_nt<T>(s, al, bl, ep, M, Co, 4 * Ci, 4, ws, st);
}
template <typename T>
size_t subpixel_ws(int B, int Hi, int Wi, int Ci, int Co) {
    return dispatch_nt_ws<T>(B * Hi * Wi, Co, 4 * Ci, 4);
}

template <typename T>
int wgrad_s2(hipStream_t s, const T* L, int B, int Hl, int Wl, int M, const T* Xh, int C, float* dW, Ws ws,
             XAcc bias_acc, float* dbias) {
    constexpr int V = Vec16<T>::N;
    HLMC_CHECK_ARG(!dbias || bias_acc.on(), "wgrad_s2: a bias gradient needs its accumulator");
    HLMC_CHECK_ARG(M % V == 0 && C % V == 0, "wgrad_s2: channel counts must be multiples of the vector width");
    const int K = B * Hl * Wl, N = 9 * C;
    StoreWgradConv ep{dW, C, bias_acc, dbias};
    probe::site(probe::kWgradS2, 2.0 * M * N * K,
                (double)sizeof(T) * ((double)K * M + 4.0 * K * C) + 4.0 * M * N);
    // power-of-two sides / channels and operands under 2 GB (every layer of the model): the buffer-descriptor loaders
    const double lbytes = (double)K * M * sizeof(T), xbytes = 4.0 * K * C * sizeof(T);
    const int lh = log2_exact(Hl), lw = log2_exact(Wl), lc = log2_exact(C), lm = log2_exact(M);
    if (lh >= 0 && lw >= 0 && lc >= 0 && lm >= 0 && lbytes < 2147483000.0 && xbytes < 2147483000.0 && aligned16(L) &&
        aligned16(Xh)) {
        KRowDenseP2<T> ll{L, lm, K, M, (uint32_t)lbytes};
        KRowConvS2P2<T> hl{Xh, lh, lw, lc, K, (uint32_t)xbytes};
        return dispatch_tn<T>(s, ll, hl, ep, M, N, K, ws);
    }
    KRowDense<T> ll{{}, L, M, K, M, aligned16(L)};
    KRowConvS2<T> hl{{}, Xh, Hl, Wl, C, K, FastDiv((uint32_t)Wl), FastDiv((uint32_t)Hl)};
    return dispatch_tn<T>(s, ll, hl, ep, M, N, K, ws);
}
template <typename T>
size_t wgrad_s2_ws(int B, int Hl, int Wl, int M, int C) {
    return dispatch_tn_ws<T>(M, 9 * C, B * Hl * Wl);
}

template <typename T, typename OutT>
int linear(hipStream_t s, const T* x, int ldx, int M, int K, const T* w, int ldw, const float* bias, int N, OutT* y,
           int ldy, int act, int accumulate, Ws ws, const OutT* relu_ref, const NhwcOut* no) {
    constexpr int V = Vec16<T>::N;
    bool vx = (ldx % V == 0) && aligned16(x);
    bool vw = (ldw % V == 0) && aligned16(w);
    DenseLoader<T> al{x, ldx, M, K, vx};
    DenseLoader<T> bl{w, ldw, N, K, vw};
    StoreRM<OutT> ep{y, bias, ldy, act, accumulate};
    probe::site(probe::kLinear, 2.0 * M * N * K, (double)sizeof(T) * ((double)M * K + (double)N * K) + (double)sizeof(OutT) * M * N);
    if (no) {  // the first ncut columns in NHWC order for the conv that reads them
        HLMC_CHECK_ARG(!relu_ref && no->nhwc && no->ncut == no->hw * no->C && no->ncut <= N, "linear: NHWC output");
        StoreFlatAsNhwc<OutT> en;
        static_cast<StoreRM<OutT>&>(en) = ep;
        en.nhwc = static_cast<OutT*>(no->nhwc);
        en.ncut = no->ncut;
        en.fx = FlatIdx(no->hw, no->C, 0);
        return dispatch_linear<T>(s, al, bl, en, M, N, K, ws);
    }
    if (relu_ref) {
        HLMC_CHECK_ARG(act == 0, "linear: a ReLU-backward mask and a forward activation together");
        StoreReluBwd<OutT> em;
        static_cast<StoreRM<OutT>&>(em) = ep;
        em.relu_ref = relu_ref;
        return dispatch_linear<T>(s, al, bl, em, M, N, K, ws);
    }
    return dispatch_linear<T>(s, al, bl, ep, M, N, K, ws);
}
template <typename T>
size_t linear_ws(int M, int K, int N) {
    return dispatch_linear_ws<T>(M, N, K);
}

template <typename T>
int linear_partials(hipStream_t s, const T* x, int ldx, int M, int K, const T* w, int ldw, int N, Ws ws, int* S_out) {
    constexpr int V = Vec16<T>::N;
    DenseLoader<T> al{x, ldx, M, K, (ldx % V == 0) && aligned16(x)};
    DenseLoader<T> bl{w, ldw, N, K, (ldw % V == 0) && aligned16(w)};
    probe::site(probe::kLinear, 2.0 * M * N * K, (double)sizeof(T) * ((double)M * K + (double)N * K) + 4.0 * M * N);
    return dispatch_linear_partials<T>(s, al, bl, M, N, K, ws, S_out);
}
template <typename T>
size_t linear_partials_ws(int M, int K, int N) {
    return std::max(dispatch_linear_ws<T>(M, N, K), (size_t)M * N * sizeof(float));
}

// Final epilogue of a dense weight gradient whose H operand carries the ones column: C[n][k < K] -> dW[n][k],
// C[n][K] -> db[n] (the bias gradient, a column sum of dy, from the same GEMM and split-K reduction).
struct StoreWgradBias {
    static constexpr bool kDirectTn = true;  // gemm_tn_kernel may store through it directly (TnDirect)
    float* dW;
    float* db;
    int K;
    struct Row {
        float* r;
        int m;
    };
    __device__ void set_phase(int) {}
    __device__ Row row(int m) const { return Row{dW + (int64_t)m * K, m}; }
    __device__ void store(const Row& rw, int n, float v) const {
        if (n < K) rw.r[n] = v;
        else db[rw.m] = v;
    }
};

template <typename T>
int linear_wgrad(hipStream_t s, const T* dy, int lddy, const T* x, int ldx, int Mb, int N, int K, float* dW, float* db,
                 Ws ws) {
    constexpr int V = Vec16<T>::N;
    KRowDense<T> ll{{}, dy, lddy, Mb, N, (lddy % V == 0) && aligned16(dy), false};
    KRowDense<T> hl{{}, x, ldx, Mb, K, (ldx % V == 0) && aligned16(x), db != nullptr};
    probe::site(probe::kLinearWgrad, 2.0 * N * K * Mb, (double)sizeof(T) * ((double)Mb * N + (double)Mb * K) + 4.0 * N * K);
    if (db) return dispatch_tn<T>(s, ll, hl, StoreWgradBias{dW, db, K}, N, K + 1, Mb, ws);
    StoreRM<float> ep{dW, nullptr, K, 0, 0};
    return dispatch_tn<T>(s, ll, hl, ep, N, K, Mb, ws);
}
// StoreWgradBias for two layers stacked along n (the latent heads' one weight-gradient GEMM): rows n < N1 belong to
// the first layer, the others to the second (their gradients are not adjacent in the flat gradient)
struct StoreWgradBiasPair {
    static constexpr bool kDirectTn = true;
    float *dW1, *db1, *dW2, *db2;
    int K, N1;
    struct Row {
        float* r;
        float* b;
    };
    __device__ void set_phase(int) {}
    __device__ Row row(int m) const {
        return m < N1 ? Row{dW1 + (int64_t)m * K, db1 + m} : Row{dW2 + (int64_t)(m - N1) * K, db2 + (m - N1)};
    }
    __device__ void store(const Row& rw, int n, float v) const {
        if (n < K) rw.r[n] = v;
        else *rw.b = v;
    }
};

template <typename T>
int linear_wgrad_pair(hipStream_t s, const T* dy, int lddy, const T* x, int ldx, int Mb, int N1, int K, float* dW1,
                      float* db1, float* dW2, float* db2, Ws ws) {
    constexpr int V = Vec16<T>::N;
    HLMC_CHECK_ARG(dW1 && db1 && dW2 && db2, "linear_wgrad_pair: gradients required");
    const int N = 2 * N1;
    KRowDense<T> ll{{}, dy, lddy, Mb, N, (lddy % V == 0) && aligned16(dy), false};
    KRowDense<T> hl{{}, x, ldx, Mb, K, (ldx % V == 0) && aligned16(x), true};
    probe::site(probe::kLinearWgrad, 2.0 * N * K * Mb, (double)sizeof(T) * ((double)Mb * N + (double)Mb * K) + 4.0 * N * K);
    return dispatch_tn<T>(s, ll, hl, StoreWgradBiasPair{dW1, db1, dW2, db2, K, N1}, N, K + 1, Mb, ws);
}

template <typename T>
size_t linear_wgrad_ws(int Mb, int N, int K) {  // with or without the bias column
    return std::max(dispatch_tn_ws<T>(N, K, Mb), dispatch_tn_ws<T>(N, K + 1, Mb));
}

#define INST(T)                                                                                                     \
    template int conv_s2<T>(hipStream_t, const T*, int, int, int, int, const T*, const float*, int, T*, Ws,         \
                            ColStats*, const BnInput*, const FlatOut*);                                             \
    template bool conv_s2_takes_input_bn<T>(int, int, int, int, int);                                              \
    template bool subpixel_takes_input_bn<T>(int, int, int, int, int);                                             \
    template size_t conv_s2_ws<T>(int, int, int, int, int);                                                        \
    template int subpixel<T>(hipStream_t, const T*, int, int, int, int, const T*, const float*, int, T*, Ws,        \
                             ColStats*, const BnInput*);                                                                             \
    template size_t subpixel_ws<T>(int, int, int, int, int);                                                       \
    template int wgrad_s2<T>(hipStream_t, const T*, int, int, int, int, const T*, int, float*, Ws, XAcc, float*);  \
    template size_t wgrad_s2_ws<T>(int, int, int, int, int);                                                       \
    template int linear<T, T>(hipStream_t, const T*, int, int, int, const T*, int, const float*, int, T*, int, int, \
                              int, Ws, const T*, const NhwcOut*);                                                  \
    template size_t linear_ws<T>(int, int, int);                                                                   \
    template int linear_partials<T>(hipStream_t, const T*, int, int, int, const T*, int, int, Ws, int*);           \
    template size_t linear_partials_ws<T>(int, int, int);                                                          \
    template int linear_wgrad_pair<T>(hipStream_t, const T*, int, const T*, int, int, int, int, float*, float*,    \
                                      float*, float*, Ws);                                                         \
    template int linear_wgrad<T>(hipStream_t, const T*, int, const T*, int, int, int, int, float*, float*, Ws);    \
    template size_t linear_wgrad_ws<T>(int, int, int);

INST(float)
INST(bf16)
#undef INST
template int linear<bf16, float>(hipStream_t, const bf16*, int, int, int, const bf16*, int, const float*, int, float*,
                                 int, int, int, Ws, const float*, const NhwcOut*);

}  // namespace ops
}  // namespace hlmc
#ifdef HLMC_TN_TS
extern "C" int hlmc_debug_tn_ts(void* host, int nblocks) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(hlmc::g_tn_ts), (size_t)nblocks * 32, 0, hipMemcpyDeviceToHost);
}
#endif
