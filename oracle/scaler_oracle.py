"""TEST INFRASTRUCTURE ONLY (checker, never shipped or measured): exact / float64 restatements of the tail of
csrc/features.hip -- the StandardScaler passes (hlmc_colstats_sum / _centered, hlmc_zscore_apply), the mean / std
pooling (hlmc_row_mean_std) and the generic librosa.power_to_db (hlmc_power_to_db) -- each with a bound on what a
correct kernel may differ by, counted from the roundings the kernel's number formats allow (u64 = 2^-53 for the
float64 accumulators, u32 = 2^-24 for a float32 result), never from a kernel's output.

Pinned on the CPU in tests/test_oracle_cpu.py: the statistics and the transform against live sklearn, and float32 /
float64 restatements of the kernels against the bounds, on every input of tests/test_scaler_ops_gpu.py.
"""
from __future__ import annotations

import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
LOG10F_ULP = 2   # accuracy assumed for the device log10f, in ulp (the ROCm install documents none)
LD = np.longdouble   # 64-bit mantissa on x86: n 2^-64 sum |x| is 2^-11 of the float64 bounds below


def sums_exact(A):
    """A = |x| of float32 values as float64 [n][cols] -> bool [cols]: every float64 partial sum of the column, in any
    order, is exact.  Each x is a multiple of q = the float32 spacing at the smallest non-zero |x| of the column
    (2^-149 at least), and so is every partial sum, none larger than sum|x|: with sum|x| <= 2^53 q they all fit the
    53-bit significand."""
    nz = np.where(A > 0, A, np.inf)
    _, e = np.frexp(nz.min(0))                                   # min = m 2^e, m in [0.5, 1): spacing 2^(e - 24)
    q = np.where(np.isfinite(nz.min(0)), np.ldexp(1.0, np.maximum(e - 24, -149)), np.inf)
    return A.sum(0) * (1 + 2.0 ** -40) <= 2.0 ** 53 * q


def col_sums(X):
    """(sum[c], bound[c]): column sums of the float32 rows, exact to longdouble.  Bound 0 where float64 partial sums are
    exact in any order (sums_exact: most float32 columns of a few thousand rows), else n u64 sum|x| + u64 |sum| (n - 1
    additions in any order, the reference's own rounding)."""
    X = np.asarray(X, dtype=np.float32)
    A = np.abs(X.astype(np.float64))
    s = X.astype(LD).sum(0).astype(np.float64)
    return s, np.where(sums_exact(A), 0.0, X.shape[0] * U64 * A.sum(0) + U64 * np.abs(s))


def col_centered(X, mean):
    """(corr, corr_bound, m2, m2_bound) for corr[c] = sum_i (x - mean), m2[c] = sum_i (x - mean)^2 with the float64
    mean as given.  Each difference is rounded once (u64 |t|) before n - 1 additions: (n + 1) u64 sum|t|; each square
    carries 2 u64 from its difference and one of its own: (n + 3) u64 m2."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    t = X.astype(LD) - np.asarray(mean, dtype=np.float64).astype(LD)[None, :]
    corr = t.sum(0).astype(np.float64)
    m2 = (t * t).sum(0).astype(np.float64)
    at = np.abs(t).sum(0).astype(np.float64)
    return corr, (n + 1) * U64 * at + U64 * np.abs(corr), m2, (n + 3) * U64 * m2 + U64 * m2


def scaler_stats(n, col_sum, corr, m2):
    """sklearn _incremental_mean_and_var on a first fit (last_sum = last_variance = 0): mean = sum / n,
    var = (m2 - corr^2 / n) / n; scale = sqrt(var), 1 where the column is near-constant (_is_constant_feature:
    var <= n eps var + (n mean eps)^2)."""
    N = float(n)
    mean = np.asarray(col_sum, dtype=np.float64) / N
    var = (np.asarray(m2, dtype=np.float64) - np.asarray(corr, dtype=np.float64) ** 2 / N) / N
    eps = np.finfo(np.float64).eps
    upper = N * eps * var + (N * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[var <= upper] = 1.0
    return mean, var, scale


def scaler_fit(X):
    """mean_, var_, scale_ of StandardScaler().fit(X) from the exact pass outputs."""
    X = np.asarray(X, dtype=np.float32)
    s, _ = col_sums(X)
    corr, _, m2, _ = col_centered(X, s / float(X.shape[0]))
    return scaler_stats(X.shape[0], s, corr, m2)


def zscore(x, mean, scale):
    """StandardScaler.transform on float32 data: X -= mean_ (float64 op, stored float32), X /= scale_ (the same)."""
    a = (np.asarray(x, dtype=np.float32).astype(np.float64) - mean).astype(np.float32)
    return (a.astype(np.float64) / scale).astype(np.float32)


def row_mean_std(x):
    """(mean, mean_bound, std, std_bound) of each row (ddof = 0).  The kernel is a float64 two-pass rounded once to
    float32: u32 |ref| for that rounding + cols 2^-52 mean|x| for the float64 sums (cols u64 sum|x| / cols on the
    mean; the same amount moves every difference, hence the std by no more, plus its own cols u64 std)."""
    x = np.asarray(x, dtype=np.float32)
    cols = x.shape[-1]
    xl = x.astype(LD)
    m = xl.mean(-1)
    sd = np.sqrt(((xl - m[..., None]) ** 2).mean(-1))
    m, sd = m.astype(np.float64), sd.astype(np.float64)
    slack = cols * 2.0 ** -52 * np.abs(x.astype(np.float64)).mean(-1)
    return m, U32 * np.abs(m) + slack, sd, U32 * np.abs(sd) + slack


def row_mean_std_f64(x):
    """The kernel's arithmetic restated: float64 two-pass, one float32 rounding."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x.sum(-1) / x.shape[-1]
    return m.astype(np.float32), np.sqrt(((x - m[..., None]) ** 2).sum(-1) / x.shape[-1]).astype(np.float32)


def power_to_db(S, ref_max=True, ref_value=1.0, amin=1e-10, top_db=80.0):
    """(out, bound, clamped) for librosa.power_to_db per clip of S [B][per] in float64:
    out = 10 log10(max(amin, S)) - 10 log10(max(amin, ref)), ref = the clip maximum or |ref_value|, then
    max(out, out.max() - top_db).  amin and ref_value are taken at their float32 values, as the kernel receives them.

    Bound: each 10 log10f carries L ulp of log10f and one rounding of the product, the difference one more:
    u32 ((L + 1)(|db_S| + |db_ref|) + |out|).  The clamp is a maximum (1-Lipschitz) against the floor, which
    carries the bound of the largest element and one rounding of its own subtraction."""
    S = np.asarray(S, dtype=np.float32).astype(np.float64)
    a = float(np.float32(amin))
    db_s = 10.0 * np.log10(np.maximum(a, S))
    ref = S.max(1) if ref_max else np.full(S.shape[0], abs(float(np.float32(ref_value))))
    db_ref = 10.0 * np.log10(np.maximum(a, ref))[:, None]
    out = db_s - db_ref
    bound = U32 * ((LOG10F_ULP + 1) * (np.abs(db_s) + np.abs(db_ref)) + np.abs(out))
    clamped = np.zeros(out.shape, dtype=bool)
    if top_db is not None:
        top = out.argmax(1)
        rows = np.arange(out.shape[0])
        floor = out[rows, top] - float(np.float32(top_db))
        floor_b = bound[rows, top] + U32 * np.abs(floor)
        clamped = out < floor[:, None] - bound - floor_b[:, None]      # below the floor whatever the roundings
        bound =np.where(out <= floor[:, None] + bound + floor_b[:, None], np.maximum(bound, floor_b[:, None]), bound)
        out = np.maximum(out, floor[:, None])
    return out, bound, clamped


def power_to_db_f32(S, ref_max=True, ref_value=1.0, amin=1e-10, top_db=80.0):
    """The kernel's float32 arithmetic with numpy's float32 log10 in the place of the device log10f."""
    S = np.asarray(S, dtype=np.float32)
    a = np.float32(amin)
    ten = np.float32(10.0)
    ref = S.max(1) if ref_max else np.full(S.shape[0], np.abs(np.float32(ref_value)), dtype=np.float32)
    ref_db = (ten * np.log10(np.maximum(a, ref)))[:, None]
    out = ten * np.log10(np.maximum(a, S)) - ref_db
    if top_db is not None:
        smax = np.maximum(S.max(1), np.float32(0))
        floor = (ten * np.log10(np.maximum(a, smax)))[:, None] - ref_db - np.float32(top_db)
        out = np.maximum(out, floor)
    return out.astype(np.float32)
