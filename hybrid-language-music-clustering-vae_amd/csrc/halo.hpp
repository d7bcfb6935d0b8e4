// Persistent LDS halo-tile kernels (bf16): the stride-2 3x3 conv and the sub-pixel (stride-2 transposed 3x3) conv of
// the four layer shapes whose input rows fit one 16-byte chunk per thread.  One kernel skeleton (halo_kernel) walks
// the tiles; a geometry policy (ConvS2Halo / SubpixelHalo) says which input rows a tile stages and which taps read
// them.  Launched from gemm_ops.hip (kConvHalo / kSubpixelHalo).
#pragma once
#include "gemm.hpp"
#include "ops.hpp"

namespace hlmc {

// The epilogue of the halo kernels: the block's bias columns from an LDS table (filled once before the tile loop)
// and stores without the accumulate read, so the tile loop issues no global loads besides the prefetched input rows.
// (With the per-tile bias / accumulate loads in the loop the compiler's wait-count merge at the loop head waited for
// ALL outstanding loads -- the prefetch included -- before the first MFMA of every tile.)
template <class EP>
struct HaloEp : EP {
    const float* lb;  // LDS: bias of columns nbase ..
    int nbase;
    __device__ float colbias(int n) const { return lb[n - nbase]; }
    __device__ float put(int64_t ro, int n, float v) const { return EP::put_na(ro, n, v); }
};

// ---- train-mode BatchNorm + LeakyReLU(0.01) of a halo kernel's INPUT, applied while its rows are staged (XIN,
// ops::BnInput): the input pointer is the pre-BN map y of the layer below; the block folds that layer's statistics
// accumulator in its prologue (bn_act_train's consumer-side finalize: bn_train_channel, block 0 stores mean / invstd /
// running statistics), transforms each staged 16-byte chunk (8 channels) in registers, and writes the activation a of
// the rows its tile owns (every input row exactly once over the grid, by the first channel-split block) for the
// weight gradient that reads it later.  Rows outside the image stay zero (padding).
template <int CI>
struct BnInLds {  // prologue scratch + per-channel parameters (LDS)
    double tot[2 * CI];
    long long red[3 * 256];
    float prm[4 * CI];  // mean | invstd | gamma | beta
};
template <int CI>
__device__ __forceinline__ void bn_in_prologue(const ops::BnInput& f, BnInLds<CI>& L) {
    xacc_fold(f.acc, L.tot, L.red);
    for (int c = threadIdx.x; c < CI; c += 256) {
        bn_train_channel(f, c, L.tot[c], L.tot[CI + c], L.prm[c], L.prm[CI + c]);
        L.prm[2 * CI + c] = f.gamma[c];
        L.prm[3 * CI + c] = f.beta[c];
    }
    __syncthreads();
}
// lrelu((x - mean) * invstd * gamma + beta) of 8 bf16 channels (the thread's parameters in registers)
__device__ __forceinline__ uint4 bn_in_apply(uint4 v, const float (&pr)[4][8]) {
    float x[8];
    cvt16_f32<bf16>(v, x);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float z = (x[k] - pr[0][k]) * pr[1][k] * pr[2][k] + pr[3][k];
        x[k] = z > 0.f ? z : 0.01f * z;
    }
    uint4 o;
    unsigned* w = reinterpret_cast<unsigned*>(&o);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bf16 lo = __float2bfloat16(x[2 * i]), hi = __float2bfloat16(x[2 * i + 1]);
        w[i] = (unsigned)(*reinterpret_cast<unsigned short*>(&lo)) | ((unsigned)(*reinterpret_cast<unsigned short*>(&hi)) << 16);
    }
    return o;
}

// ---- what the geometries share.  CI input channels, COB output channels per block (NSPL blocks share a tile's
// Co = NSPL * COB); a staged pixel is CI + 8 bf16 apart from the next and a weight row 9 CI + 8, so the 16 rows of a
// fragment are read from distinct 16-byte LDS slots.
template <int CI_, int COB_, int NSPL_>
struct HaloDims {
    static constexpr int CI = CI_, COB = COB_, NSPL = NSPL_, CO = NSPL_ * COB_;
    static constexpr int CPP = CI / 8, PS = CI + 8, KP = 9 * CI + 8;  // chunks per pixel, pixel / weight-row pitch
};
// One tap of a wave's TM x TN grid of 16 x 16 tiles: the A fragments from the staged halo H (pix(m): the staged
// pixel, row * HC + column, that the tile's output pixel m reads for this tap), the B fragments from column block
// `tap` of the weight rows Bs.  The wave's tiles start at pixel wm0 / channel wn0 of the block's TP x COB tile.
template <class G, class PIX>
__device__ __forceinline__ void halo_tap(const bf16* H, const bf16* Bs, int tap, int wm0, int wn0, int lane, PIX pix,
                                         f32x4_t (&acc)[G::TM][G::TN]) {
    const int g8 = (lane >> 4) * 8;
#pragma unroll
    for (int kc = 0; kc < G::CI / 32; ++kc) {
        bf16x8_t af[G::TM], bfr[G::TN];
#pragma unroll
        for (int i = 0; i < G::TM; ++i) {
            const int m = wm0 + i * 16 + (lane & 15);
            af[i] = *reinterpret_cast<const bf16x8_t*>(&H[pix(m) * G::PS + kc * 32 + g8]);
        }
#pragma unroll
        for (int j = 0; j < G::TN; ++j) {
            const int n = wn0 + j * 16 + (lane & 15);
            bfr[j] = *reinterpret_cast<const bf16x8_t*>(&Bs[n * G::KP + tap * G::CI + kc * 32 + g8]);
        }
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
#pragma unroll
            for (int j = 0; j < G::TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
}
template <class G>
__device__ __forceinline__ void halo_zero(f32x4_t (&acc)[G::TM][G::TN]) {
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
        for (int j = 0; j < G::TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}
// Stores the wave's tiles (rows mb .., columns nb ..) with the per-element epilogue and, kStatMode 1, adds the
// stored values' column sums to the lane's running statistics.  (The transposed-accumulator epilogue of the
// split-K GEMMs, epilogue_tile_t, made these kernels 4-15 % slower: gemm_ops.hip nt_kernel_launch_tr.)
template <class G, class HEP>
__device__ __forceinline__ void halo_store(const HEP& hep, const f32x4_t (&acc)[G::TM][G::TN], int mb, int nb, int lane,
                                           int M, double (&run_s)[G::TN], double (&run_q)[G::TN]) {
    double cs[G::TN], cq[G::TN];
    epilogue_tile<G::TM, G::TN>(hep, acc, mb, nb, lane, M, G::CO, cs, cq);
    if constexpr (HEP::kStatMode == 1) {
#pragma unroll
        for (int j = 0; j < G::TN; ++j) {
            run_s[j] += cs[j];
            run_q[j] += cq[j];
        }
    }
}

// ---- geometry policies.  Constants: WI staged input width (WI * CPP == 256: one 16-byte chunk per thread per input
// row), HR x HC staged rows x columns, PADC the zero column and COL0 the staged column of input column 0, TP tile
// pixels (M rows of the GEMM), the 4 waves as (4 / WAVES_N) x WAVES_N over TP x COB with TM x TN 16 x 16 tiles each.
// Functions: tiles_per_image; in_row / inside / clamped (the input row that staged row u of an image's tile ti
// holds, whether it lies in the image, and the in-image row loaded in its place); PADU / pads (the one staged row
// that can lie outside, and whether it does for tile ti: it is then staged as zero padding); owns (the rows a tile
// writes to a_out); compute (the MFMA body and its epilogues); block_total (the cross-wave sum of a column's
// statistics: its association is part of the result's bits).

// Stride-2 3x3 conv, WO output width, ROWS output rows per tile: a tile's 2 ROWS + 1 input rows (plus the zero
// column left of the image) are staged once and every tap's A fragment is read from there, so the input crosses L2
// once per tile instead of once per (tap, 16-byte chunk) gather.
// Measured (scripts/bench_gemm.py): the 64x64x32 -> 64 conv and the matching decoder data gradient 46.3 / 44.1 ->
// 36.7 / 34.2 us; bench A/B 106.4k vs 105.0k clips/s (3 alternating rounds).
template <int CI_, int COB_, int NSPL_, int WO, int ROWS>
struct ConvS2Halo : HaloDims<CI_, COB_, NSPL_> {
    static constexpr int WI = 2 * WO, HR = 2 * ROWS + 1, HC = WI + 1, PADC = 0, COL0 = 1, TP = ROWS * WO;
    static constexpr int WAVES_N = COB_ / 32;  // 2 x 2 waves over (TP x 64) or 4 x 1 over (TP x 32)
    static constexpr int TM = TP / (4 / WAVES_N) / 16, TN = 2;
    static_assert(COB_ == 64 || COB_ == 32, "wave tiling");
    __device__ __forceinline__ static int tiles_per_image(int Hi) { return (Hi / 2) / ROWS; }
    // row -1 lies above the image
    __device__ __forceinline__ static int in_row(int ti, int u) { return 2 * (ti * ROWS) - 1 + u; }
    __device__ __forceinline__ static bool inside(int ih, int) { return ih >= 0; }
    __device__ __forceinline__ static int clamped(int ih, int) { return ih < 0 ? 0 : ih; }
    static constexpr int PADU = 0;
    __device__ __forceinline__ static bool pads(int ti, int) { return ti == 0; }
    __device__ __forceinline__ static bool owns(int u) { return u > 0; }  // rows 2 oh0 .. 2 oh0 + 2 ROWS - 1
    template <class HEP>
    __device__ __forceinline__ static void compute(const bf16* H, const bf16* Bs, const HEP& hep, int mb, int nb,
                                                   int wm0, int wn0, int lane, int M, double (&run_s)[TN],
                                                   double (&run_q)[TN]) {
        f32x4_t acc[TM][TN];
        halo_zero<ConvS2Halo>(acc);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;  // input (2oh-1+kh, 2ow-1+kw), staged one column to the right
            halo_tap<ConvS2Halo>(H, Bs, tap, wm0, wn0, lane,
                                 [&](int m) { return (2 * (m / WO) + kh) * HC + 2 * (m % WO) + kw; }, acc);
        }
        halo_store<ConvS2Halo>(hep, acc, mb, nb, lane, M, run_s, run_q);
    }
    __device__ __forceinline__ static double block_total(const double (*sred)[2][COB_], int k, int c) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < 4 / WAVES_N; ++w) a += sred[w][k][c];
        return a;
    }
};

// Sub-pixel conv, WI low-res width, ROWS low-res rows per tile (TP = ROWS * WI = 128 low-res pixels): a tile's
// ROWS + 1 input rows (its own plus the next, and a zero column right of the image) are staged once, and all 4
// phases' taps (1 + 2 + 2 + 4) read their fragments from there; each phase has its own epilogue.
template <int CI_, int COB_, int NSPL_, int WI_, int ROWS>
struct SubpixelHalo : HaloDims<CI_, COB_, NSPL_> {
    static constexpr int WI = WI_, HR = ROWS + 1, HC = WI + 1, PADC = WI, COL0 = 0, TP = ROWS * WI;
    static constexpr int WAVES_N = 1, TM = 2, TN = COB_ / 16;  // 4 waves x (32 pixels x COB channels)
    static_assert(TP == 128 && (COB_ == 32 || COB_ == 16), "wave tiling");
    __device__ __forceinline__ static int tiles_per_image(int Hi) { return Hi / ROWS; }
    // row Hi lies below the image
    __device__ __forceinline__ static int in_row(int ti, int u) { return ti * ROWS + u; }
    __device__ __forceinline__ static bool inside(int ih, int Hi) { return ih < Hi; }
    __device__ __forceinline__ static int clamped(int ih, int Hi) { return ih < Hi ? ih : Hi - 1; }
    static constexpr int PADU = ROWS;
    __device__ __forceinline__ static bool pads(int ti, int tpi) { return ti == tpi - 1; }
    __device__ __forceinline__ static bool owns(int u) { return u < ROWS; }
    template <class HEP>
    __device__ __forceinline__ static void compute(const bf16* H, const bf16* Bs, const HEP& hep, int mb, int nb,
                                                   int wm0, int wn0, int lane, int M, double (&run_s)[TN],
                                                   double (&run_q)[TN]) {
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const int py = ph >> 1, px = ph & 1;
            f32x4_t acc[TM][TN];
            halo_zero<SubpixelHalo>(acc);
#pragma unroll
            for (int ty = 0; ty < 2; ++ty) {
                if (ty == 1 && !py) continue;
                const int kh = py ? (ty ? 2 : 0) : 1, dr = (py && ty == 0) ? 1 : 0;
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    if (tx == 1 && !px) continue;
                    const int kw = px ? (tx ? 2 : 0) : 1, dc = (px && tx == 0) ? 1 : 0;
                    halo_tap<SubpixelHalo>(H, Bs, kh * 3 + kw, wm0, wn0, lane,
                                           [&](int m) { return (m / WI + dr) * HC + m % WI + dc; }, acc);
                }
            }
            HEP e = hep;
            e.set_phase(ph);
            halo_store<SubpixelHalo>(e, acc, mb, nb, lane, M, run_s, run_q);
        }
    }
    __device__ __forceinline__ static double block_total(const double (*sred)[2][COB_], int k, int c) {
        return (sred[0][k][c] + sred[1][k][c]) + (sred[2][k][c] + sred[3][k][c]);
    }
};

// ---- the persistent tile walk.  A block (NSPL of them per tile, one channel split each) keeps its COB packed
// weight rows [9 x CI] in LDS and walks the tiles t = blockIdx.x / NSPL, + gridDim.x / NSPL, ...; each tile's HR
// input rows are staged in LDS once (one buffer: the barrier pair at the end of a tile is covered by the co-resident
// block or costs less than a second buffer's LDS), and the next tile's rows are loaded into registers while this
// tile computes.  EP: the output epilogue (kStatMode 1: WithStats, column statistics of the stored values into its
// exact accumulator); XIN: the input BatchNorm above (xin; else ignored); WPE: waves per SIMD the register
// allocation targets (2: two blocks per CU where the LDS allows).
template <class G, class EP, bool XIN, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void halo_kernel(
    const bf16* __restrict__ x, int Hi, int ntiles, const bf16* __restrict__ wp, EP ep, int M, ops::BnInput xin) {
    constexpr int CI = G::CI, COB = G::COB, NSPL = G::NSPL, CPP = G::CPP, PS = G::PS, KP = G::KP;
    constexpr int WI = G::WI, HR = G::HR, HC = G::HC, TN = G::TN, WAVES_N = G::WAVES_N, WAVES_M = 4 / WAVES_N;
    static_assert(WI * CPP == 256 && WAVES_M * G::TM * 16 == G::TP && WAVES_N * TN * 16 == COB,
                  "halo chunk map / wave tiling");
    __shared__ __attribute__((aligned(16))) bf16 Bs[COB * KP];
    __shared__ __attribute__((aligned(16))) bf16 Hs[HR * HC * PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WAVES_N) * (G::TM * 16), wn0 = (wave % WAVES_N) * (TN * 16);
    const int tpi = G::tiles_per_image(Hi);
    const int nh = blockIdx.x % NSPL, n0 = nh * COB;
    const int bstep = gridDim.x / NSPL;
    __shared__ float bsh[COB];  // this block's bias columns
    if (tid < COB) bsh[tid] = n0 + tid < G::CO ? ep.colbias(n0 + tid) : 0.f;
    HaloEp<EP> hep;
    static_cast<EP&>(hep) = ep;
    hep.lb = bsh;
    hep.nbase = n0;
    for (int c = tid; c < COB * 9 * CPP; c += 256) {  // this block's weight rows
        const int n = c / (9 * CPP), q = c - n * (9 * CPP);
        *reinterpret_cast<uint4*>(&Bs[n * KP + q * 8]) =
            *reinterpret_cast<const uint4*>(wp + (int64_t)(n0 + n) * 9 * CI + q * 8);
    }
    for (int c = tid; c < HR * CPP; c += 256) {  // the pad column (input column -1 / WI) stays zero
        const int r = c / CPP, q = c - r * CPP;
        *reinterpret_cast<uint4*>(&Hs[(r * HC + G::PADC) * PS + q * 8]) = make_uint4(0, 0, 0, 0);
    }
    uint4 hr[HR];  // HR rows x 256 chunks / 256 threads
    auto row_off = [&](int b, int ih) { return (((int64_t)b * Hi + ih) * WI + tid / CPP) * CI + (tid % CPP) * 8; };
    // unconditional loads (a row outside the image clamped to one inside; zeroed when staged): a branch per row made
    // the compiler wait for the loads right after issuing them
    auto load_rows = [&](uint4* h, int t) {
        const int b = t / tpi, ti = t - b * tpi;
#pragma unroll
        for (int u = 0; u < HR; ++u)
            h[u] = *reinterpret_cast<const uint4*>(x + row_off(b, G::clamped(G::in_row(ti, u), Hi)));
    };
    float pr[XIN ? 4 : 1][8];  // XIN: this thread's 8 channels' BatchNorm parameters
    // XIN: the rows of tile t inside the image become activations; the rows the tile owns are its to write
    auto xform_rows = [&](uint4* h, int t) {
        if constexpr (XIN) {
            const int b = t / tpi, ti = t - b * tpi;
#pragma unroll
            for (int u = 0; u < HR; ++u) {
                const int ih = G::in_row(ti, u);
                if (!G::inside(ih, Hi)) continue;
                h[u] = bn_in_apply(h[u], pr);
                if (G::owns(u) && nh == 0)
                    *reinterpret_cast<uint4*>(static_cast<bf16*>(xin.a_out) + row_off(b, ih)) = h[u];
            }
        }
    };
    auto store_rows = [&](const uint4* h, int t) {
        const bool pad = G::pads(t % tpi, tpi);  // the tile's staged row PADU is zero padding above / below the image
#pragma unroll
        for (int u = 0; u < HR; ++u)
            *reinterpret_cast<uint4*>(&Hs[(u * HC + tid / CPP + G::COL0) * PS + (tid % CPP) * 8]) =
                (u == G::PADU && pad) ? make_uint4(0, 0, 0, 0) : h[u];
    };
    int t = blockIdx.x / NSPL;
    if (t < ntiles) load_rows(hr, t);  // in flight during the statistics prologue
    if constexpr (XIN) {
        __shared__ BnInLds<CI> bl;
        bn_in_prologue<CI>(xin, bl);
        const int c0 = (tid % CPP) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            pr[0][k] = bl.prm[c0 + k];
            pr[1][k] = bl.prm[CI + c0 + k];
            pr[2][k] = bl.prm[2 * CI + c0 + k];
            pr[3][k] = bl.prm[3 * CI + c0 + k];
        }
    }
    if (t < ntiles) {
        xform_rows(hr, t);
        store_rows(hr, t);
    }
    __syncthreads();
    // statistics (kStatMode 1): each lane's column sums over all its tiles (and phases) in registers, reduced across
    // the block once at the end (a per-tile LDS reduction cost two barriers per tile, per phase eight)
    double run_s[TN], run_q[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) run_s[j] = run_q[j] = 0.0;
    __shared__ double sred[EP::kStatMode == 1 ? WAVES_M : 1][2][COB];
    for (; t < ntiles; t += bstep) {
        const int tn = t + bstep;
        // in flight during this tile's MFMAs and stores; unconditional (clamped tile index, the last tile re-reads
        // its own rows): with a conditional load the compiler cannot count the loads younger than the ones it must
        // wait for and waits for all of them (measured with the bias / accumulate loads moved out of the loop:
        // 36.6 -> 27.1 us for the 64 x 64 x 32 -> 64 conv; a second register set two tiles ahead: slower)
        load_rows(hr, min(tn, ntiles - 1));
        G::compute(Hs, Bs, hep, t * G::TP + wm0, n0 + wn0, wm0, wn0, lane, M, run_s, run_q);
        if (tn < ntiles) xform_rows(hr, tn);
        __syncthreads();  // every wave is done with this tile's halo
        if (tn < ntiles) store_rows(hr, tn);
        __syncthreads();
    }
    if constexpr (EP::kStatMode == 1) {
        stats_to_lds<false, TN, COB>(run_s, run_q, &sred[0][0][0], wave / WAVES_N, wn0, lane);
        __syncthreads();
        if (tid < COB) {
            const int shard = (int)(blockIdx.x % (unsigned)ep.acc.shards);
            xacc_add_shard(ep.acc, shard, n0 + tid, G::block_total(sred, 0, tid));
            xacc_add_shard(ep.acc, shard, G::CO + n0 + tid, G::block_total(sred, 1, tid));
        }
    }
}

}  // namespace hlmc
