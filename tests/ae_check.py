"""Shared by tests/test_autoencoder_cpu.py and tests/test_autoencoder_gpu.py: the cases, inputs, numpy restatement and
bounds of hlmc_mse_rows (include/hlmc.h), so that the restatement is held on the CPU to the very bounds the kernel is
held to on the GPU.

Bounds, with u32 = 2^-24 and u64 = 2^-53 the unit roundoffs (round to nearest) and N = valid * d:

  gradient   g = fl32(fl64(fl64(r - t) * fl64(2 / N))), exact value g* = 2 (r - t) / N.
             Three float64 roundings (the difference, the quotient 2 / N -- N itself is an exact float64 -- and the
             product) and ONE float32 rounding; the yardstick, 2 (r - t) / N in float64, carries three more
             float64 roundings:  |g - g*| <= |g*| (u32 + 6.2 u64) + 2^-150  (the last term: the float32 result may be
             subnormal, spacing 2^-149).  6.2 u64 is 7e-16 against u32 = 6e-8: "one float32 rounding" to eight digits.
  sum        S = sum of fl64(fl64(r - t)^2): every term carries two roundings of the difference (squared: 2 u64) and
             one of the square, and a float64 sum of N terms in ANY order is off by at most (N - 1) u64 times the sum
             of the (non-negative) terms, to first order: (N + 2) u64 S*.  The yardstick S* used here, math.fsum of the
             float64 squares of the float64 differences, is exact but for those same three roundings per term, one of
             which may differ from the kernel's: |S - S*| <= 1.01 (N + 3) u64 S*  (1.01 covers the second-order terms
             for N < 2^40).
  count      sums2[1] = valid * d exactly (an integer below 2^53).
"""
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53

# (B, d, valid): one block / two launches, vector / scalar path (d % 4), one row, one element; valid in {1, B/2, B}
MSE_SHAPES = [(1, 1), (32, 290), (33, 13), (256, 4096)]
MSE_CASES = sorted({(B, d, v) for B, d in MSE_SHAPES for v in (1, max(1, B // 2), B)})


def mse_inputs(B, d, seed=0):
    """Seeded float32 [B][d] pair with mixed magnitudes (some rows 1e3 larger, a few exact ties r == t)."""
    rng = np.random.default_rng(1000 * B + d + seed)
    target = rng.standard_normal((B, d)).astype(np.float32)
    recon = (target + rng.standard_normal((B, d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    recon[::3] *= np.float32(1e3)
    ties = rng.random((B, d)) < 0.01
    recon[ties] = target[ties]
    return recon, target


def mse_rows_f32(recon, target, valid):
    """The kernel's arithmetic in numpy: float64 differences of the float32 inputs, one float64 scale 2 / (valid d),
    the product rounded to float32; zero rows past `valid`; the squared differences summed in float64 (numpy's pairwise
    order, not the kernel's: the bound holds for any order)."""
    B, d = recon.shape
    df = recon[:valid].astype(np.float64) - target[:valid].astype(np.float64)
    scale = 2.0 / (float(valid) * float(d))
    g = np.zeros((B, d), np.float32)
    g[:valid] = (df * scale).astype(np.float32)
    return g, np.array([np.sum(df * df), float(valid) * float(d)], np.float64)


def check_mse(recon, target, valid, g, sums):
    """Hold (g [B][d] float32, sums [2] float64) to the bounds in the module docstring.  The exact values: the
    differences of float32 numbers within 2^29 of each other in magnitude are exact in float64; in general they carry
    the one rounding the bound already counts, so the float64 difference serves as r - t."""
    B, d = recon.shape
    n = valid * d
    assert g.dtype == np.float32 and g.shape == (B, d) and sums.dtype == np.float64
    df = recon[:valid].astype(np.float64) - target[:valid].astype(np.float64)
    gstar = 2.0 * df / n
    err = np.abs(g[:valid].astype(np.float64) - gstar)
    bound = np.abs(gstar) * (U32 + 6.2 * U64) + 2.0 ** -150
    worst = float((err / bound).max())
    assert worst <= 1.0, f"d_recon: worst |err| / bound {worst:.3f}"
    pad = g[valid:].view(np.uint32)
    assert not pad.any(), "padding rows of d_recon are not +0.0f bit for bit"
    s_star = math.fsum((df * df).ravel().tolist())
    assert abs(float(sums[0]) - s_star) <= 1.01 * (n + 3) * U64 * s_star, (float(sums[0]), s_star)
    assert float(sums[1]) == float(n)
    return worst
