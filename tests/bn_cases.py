"""Case tables and float64 references of the op-level BatchNorm, fused edge-conv and latent-reduce tests
(tests/test_bn_fwd_ops_gpu.py, test_bn_bwd_ops_gpu.py, test_edge_fused_ops_gpu.py, test_latent_ops_gpu.py) and their
CPU proof against torch (tests/test_bn_cases_cpu.py).  A plain module: no GPU imports, no test functions.

Shapes are the smallest at which each index computation of the kernels changes (csrc/kernels.hip): with V = 4 (fp32)
or 8 (bf16) channels per thread a row takes tpr = C / V threads, a block pass covers rpp = 256 / tpr rows,
bn_rows_per_blk decides the block ranges, C > 512 (kFinMaxC) takes the separate finalize launch, R <= 1024 without a
mask the one-launch small backward."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
MOMENTUM, EPS = 0.1, 1e-5
MSCALE = 1.0 / 0.7          # Dropout(0.3) of the dense models
ZMIN = 1e-3                 # no |z| below this in a backward case (flip_free_y)

# ------------------------------------------------------------------------------------------------ forward cases
# (R, C) per dtype
FWD_SHAPES = {
    "fp32": [(1, 4), (255, 4), (1025, 4),                      # tpr == 1
             (3001, 32), (1500, 64), (3001, 128),              # conv layers: several blocks, the last one partial
             (2049, 512), (77, 1024),                          # around kFinMaxC; C > 512: the finalize launch
             (2, 256), (64, 512), (5, 128)],                   # BatchNorm1d rows
    "bf16": [(2, 8), (1025, 8),
             (3001, 32), (1500, 64), (3001, 128),
             (2049, 512), (77, 1024), (33, 2048),              # (33, 2048): tpr == 256, rpp == 1
             (2, 256), (64, 512), (5, 128)],
}
FWD_R1 = (1, 64)
FWD_VARIANT_SHAPES = [(3001, 32), (2049, 512), (77, 1024), (64, 512)]
FWD_FLAT = [(hw, B) for hw in (4, 6) for B in (1, 3)]          # R = B * hw, ld = C * hw + 8
FWD_FLAT_C = [32, 512, 1024]                                   # the variant shapes' channel counts
# exact-placement cases: the shapes above with even R, and the odd multi-block ones made even by one row
FWD_EXACT = {"fp32": [(1500, 64), (2, 256), (64, 512), (3002, 32), (2050, 512), (78, 1024)],
             "bf16": [(2, 8), (1500, 64), (2, 256), (64, 512), (3002, 32), (2050, 512), (78, 1024), (34, 2048)]}
# the one large case: the second iteration of bn_act_kernel's grid-stride loop (grid capped at 8192 blocks of
# rpp * kU = 256 * 4 rows at C = 4 fp32) is not reached below 8192 * 1024 rows
FWD_GRID_STRIDE = (8192 * 1024 + 3, 4)
NONFINITE = (3001, 32, 3, 5)    # R, C, the column with one NaN, the column with one +inf

# ------------------------------------------------------------------------------------------------ backward cases
# with a mask (always the two-pass kernels): (R, C, act); each at lda == C and lda == C + 16
BWD_MASKED = [(64, 512, 1), (2, 256, 1), (5, 128, 1), (1500, 64, 1), (2049, 512, 1), (77, 1024, 1),
              (1500, 64, 0), (1500, 64, 2), (77, 1024, 0), (77, 1024, 2)]
# without a mask, R <= 1024: bn_bwd_small_kernel (<T, 0> for act 0, <T, -1> else)
BWD_SMALL = [(R, C, act) for (R, C) in [(64, 512), (1024, 64), (2, 256)] for act in (0, 1, 2)]

# ------------------------------------------------------------------------------------------------ fused edge conv
EDGE_FUSED = [(1, 2, 2), (3, 6, 10), (2, 128, 128), (5, 256, 256)]   # (B, Hi, Wi)

# ------------------------------------------------------------------------------------------------ latent reduces
# (B, K, L): L % 4 != 0 takes the scalar heads_reparam instantiation; B * L % 4 != 0 leaves a partial last group and
# with L = 6 / 10 a group of four straddles two rows.  K = 200 is no multiple of 64.
LATENT = [(1, 512, 32), (3, 8192, 16), (5, 200, 10), (3, 512, 6), (5, 8192, 6), (1, 200, 10), (3, 200, 32),
          (5, 512, 10), (1, 100, 6)]
GEMM_BK = {"fp32": 32, "bf16": 64}   # gemm.hpp gemm_bk: 8 chunks of one 16-byte vector


def linear_splits(dt, M, K, N):
    """Split count of linear() / linear_partials() (gemm_ops.hip plan_nt under with_linear_tile: 64 x 64 tiles for
    M < 1024, 512 target blocks, at least two K-steps per split)."""
    assert M < 1024
    bk = GEMM_BK[dt]
    tiles = -(-M // 64) * -(-N // 64)
    S = 1
    if tiles < 256:
        S = min(-(-512 // tiles), max(1, K // (2 * bk)))
    ksl = -(-(-(-K // S)) // bk) * bk
    return -(-K // ksl)


def ld8(n):
    """Row stride of a padded latent buffer: n rounded up to 8, plus 8."""
    return (n + 7) // 8 * 8 + 8


# ------------------------------------------------------------------------------------------------ helpers
def quant(t, tdt):
    """t rounded to the kernel's dtype, as float64."""
    return t.to(tdt).to(F64)


def seed_of(*dims):
    s = 0
    for d in dims:
        s = (s * 1009 + int(d)) % (2 ** 31 - 1)
    return s


def f32(v):
    """A Python float rounded to float32 and widened again: what a kernel sees of a float argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def act_fwd(z, act):
    if act == 0:
        return torch.where(z > 0, z, 0.01 * z)
    if act == 1:
        return z.clamp_min(0)
    return z


def act_grad(z, act):
    if act == 0:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01))
    if act == 1:
        return (z > 0).to(z.dtype)
    return torch.ones_like(z)


def make_mask(gen, R, C):
    """Dropout keep mask as the kernels read it: any non-zero byte keeps; about 30 % zeros, the rest 1 or 255."""
    u = torch.rand(R, C, generator=gen)
    m = torch.where(u < 0.3, 0, 1).to(torch.uint8)
    return torch.where((u > 0.65) & (m > 0), torch.tensor(255, dtype=torch.uint8), m)


def bn_params(gen, C):
    gamma = (1 + 0.2 * torch.randn(C, generator=gen)).clamp_min(0.5)
    beta = 0.1 * torch.randn(C, generator=gen)
    rm = torch.randn(C, generator=gen)
    rv = torch.rand(C, generator=gen) + 0.5
    return gamma.float(), beta.float(), rm.float(), rv.float()


# ------------------------------------------------------------------------------------------------ BatchNorm forward
def batch_stats(y64, eps):
    """mean, biased variance, invstd over the rows of y64 (float64); eps as the kernel sees it (float32 widened:
    bn_train_finalize adds (double)eps)."""
    m = y64.mean(0)
    var = ((y64 - m) ** 2).mean(0)
    return m, var, 1.0 / torch.sqrt(var + f32(eps))


def bn_fwd_ref(y64, gamma, beta, act, eps=EPS, momentum=MOMENTUM, rm=None, rv=None, mask=None, mscale=1.0):
    """Train-mode BatchNorm + activation [+ dropout] of the quantised map y64 in float64.  Returns a dict: mean, var,
    invstd, a, absref (the per-element magnitude of assert_elementwise), rm / rv (the blended running statistics, with
    momentum as the kernel sees it, float32 widened; the unbiased variance, for R == 1 the biased value 0, as
    common.hpp bn_train_finalize documents)."""
    R = y64.shape[0]
    g, b = gamma.to(F64), beta.to(F64)
    m, var, inv = batch_stats(y64, eps)
    z = (y64 - m) * inv * g + b
    a = act_fwd(z, act)
    keep = None
    if mask is not None:
        keep = (mask != 0).to(F64) * f32(mscale)
        a = a * keep
    absref = ((y64.abs() + m.abs()) * inv * g.abs() + b.abs()) * (f32(mscale) if mask is not None else 1.0)
    out = {"mean": m, "var": var, "invstd": inv, "z": z, "a": a, "absref": absref}
    if rm is not None:
        mom = f32(momentum)
        unb = var * R / (R - 1) if R > 1 else var
        out["rm"] = (1.0 - mom) * rm.to(F64) + mom * m
        out["rv"] = (1.0 - mom) * rv.to(F64) + mom * unb
    return out


def bn_eval_ref(y64, gamma, beta, act, rm, rv, eps=EPS):
    """Eval mode: the running statistics as float32 (bn_eval_kernel computes 1 / sqrtf(rv + eps) in float32; its
    float64 value is the reference, the float32 rounding is inside the ulp tolerance)."""
    g, b = gamma.to(F64), beta.to(F64)
    m, inv = rm.to(F64), 1.0 / torch.sqrt(rv.to(F64) + f32(eps))
    z = (y64 - m) * inv * g + b
    return {"mean": m, "invstd": inv, "a": act_fwd(z, act), "absref": (y64.abs() + m.abs()) * inv * g.abs() + b.abs()}


def to_flat(a, hw):
    """[B * hw][C] NHWC rows -> [B][C * hw] NCHW-flat rows (column c * hw + p)."""
    R, C = a.shape
    return a.reshape(R // hw, hw, C).permute(0, 2, 1).reshape(R // hw, C * hw)


def exact_fwd_case(gen, R, C):
    """The exact-placement case: every column holds +2 and -2 equally often in an order drawn per column, eps = 0,
    gamma[c] = 2^(c % 4), beta[c] = c % 7 - 3: mean 0, invstd 0.5, z = +-gamma + beta a small integer."""
    assert R % 2 == 0
    order = torch.rand(R, C, generator=gen).argsort(0)
    y = torch.where(order < R // 2, 2.0, -2.0).to(F64)
    c = torch.arange(C)
    gamma = (2.0 ** (c % 4)).float()
    beta = (c % 7 - 3).float()
    return y, gamma, beta


def exact_fwd_expected(y64, gamma, beta, act, tdt, mask=None, mscale=1.0):
    """The stored activation of the exact case, reproduced rounding by rounding: z is an integer; LeakyReLU's negative
    side is float32(float32(0.01) * z); the dropout scale one more float32 multiply; one rounding to the dtype."""
    z = (y64 * 0.5 * gamma.to(F64) + beta.to(F64)).float()
    assert bool((z == z.round()).all()) and float(z.abs().max()) <= 11
    if act == 0:
        t = torch.where(z > 0, z, torch.tensor(0.01, dtype=torch.float32) * z)
    elif act == 1:
        t = z.clamp_min(0)
    else:
        t = z
    if mask is not None:
        t = torch.where(mask != 0, t * torch.tensor(mscale, dtype=torch.float32), torch.zeros_like(t))
    return t.to(tdt)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def flip_free_y(y, tdt, gamma, beta, eps=EPS, zmin=ZMIN, max_iter=200):
    """y quantised to tdt (as float64) with no element whose float64 z = xhat gamma + beta has |z| < zmin: the
    activation derivative is discontinuous at 0 and a float32 sign flip there would move a column sum by 0.99 |da|.
    Deterministic: such elements are replaced by the (quantised) value that gives z about 0.5, the statistics
    recomputed, and again until none is left.  Returns (y64, rounds)."""
    g, b = gamma.to(F64), beta.to(F64)
    yq = quant(y, tdt)
    for it in range(max_iter):
        m, _, inv = batch_stats(yq, eps)
        z = (yq - m) * inv * g + b
        bad = z.abs() < zmin
        if not bool(bad.any()):
            return yq, it
        tgt = quant((m + (0.5 - b) / (g * inv)).expand_as(yq), tdt)
        yq = torch.where(bad, tgt, yq)
    raise AssertionError("flip_free_y did not converge")


def count_near_zero(y64, gamma, beta, eps=EPS, zmin=ZMIN):
    m, _, inv = batch_stats(y64, eps)
    z = (y64 - m) * inv * gamma.to(F64) + beta.to(F64)
    return int((z.abs() < zmin).sum())


def bwd_case(dt_name, tdt, R, C, act, masked):
    """Operands of one backward case (float64 values representable in tdt; mean / invstd float32 as the forward
    stores them)."""
    gen = torch.Generator().manual_seed(seed_of(R, C, act, int(masked), dt_name == "bf16"))
    y = torch.randn(R, C, generator=gen) * 1.7 + 0.3
    da = quant(torch.randn(R, C, generator=gen), tdt)
    gamma, beta, _, _ = bn_params(gen, C)
    mask = make_mask(gen, R, C) if masked else None
    y64, _ = flip_free_y(y, tdt, gamma, beta)
    m, _, inv = batch_stats(y64, EPS)
    return {"y": y64, "da": da, "gamma": gamma, "beta": beta, "mask": mask, "mean": m.float(), "invstd": inv.float()}


def bn_bwd_ref(y64, da64, mean, invstd, gamma, beta, act, mask=None, mscale=1.0):
    """dz = da * mask * mscale * act'(z); dy = gamma invstd (dz - sum dz / R - xhat sum(dz xhat) / R);
    dgamma = sum dz xhat; dbeta = sum dz, in float64 from the float32 mean / invstd the kernel is given."""
    R = y64.shape[0]
    g, b, m, inv = gamma.to(F64), beta.to(F64), mean.to(F64), invstd.to(F64)
    xh = (y64 - m) * inv
    z = xh * g + b
    dz = da64 * act_grad(z, act)
    if mask is not None:
        dz = dz * (mask != 0).to(F64) * f32(mscale)
    s0, sx = dz.sum(0), (dz * xh).sum(0)
    dy = g * inv * (dz - s0 / R - xh * sx / R)
    return {"dy": dy, "dgamma": sx, "dbeta": s0, "dz": dz, "xhat": xh, "z": z}


# ------------------------------------------------------------------------------------------------ edge conv
def edge_bn_case(tdt, B, Hi, Wi):
    """The BatchNorm layer whose output gradient the fused edge conv (mode 2) writes: its pre-BN map ybn [R][32]
    (flip_free_y), float32 mean / invstd, gamma, beta.  |beta| >= 0.01: at R = 1 xhat is 0 and z = beta, which no
    choice of y moves away from the kink."""
    R = B * (Hi // 2) * (Wi // 2)
    gen = torch.Generator().manual_seed(seed_of(B, Hi, Wi, 32))
    gamma, beta, _, _ = bn_params(gen, 32)
    beta = torch.where(beta.abs() < 0.01, torch.full_like(beta, 0.01), beta)
    y64, _ = flip_free_y(torch.randn(R, 32, generator=gen) * 1.7 + 0.3, tdt, gamma, beta)
    m, _, inv = batch_stats(y64, EPS)
    return {"y": y64, "gamma": gamma, "beta": beta, "mean": m.float(), "invstd": inv.float()}


def conv_c1_ref(x64, w64, b64):
    """Conv2d(1, 32, 3, stride 2, padding 1) of x [B, H, W] -> NHWC [B, H / 2, W / 2, 32], float64."""
    return F.conv2d(x64[:, None], w64, b64, stride=2, padding=1).permute(0, 2, 3, 1).contiguous()


def conv_c1_plain(x64, w64, b64):
    """The same sum written out tap by tap (tests/test_bn_cases_cpu.py compares the two)."""
    B, H, W = x64.shape
    xp = F.pad(x64, (1, 1, 1, 1))
    out = b64.reshape(1, 1, 1, -1).expand(B, H // 2, W // 2, w64.shape[0]).clone()
    for kh in range(3):
        for kw in range(3):
            tap = xp[:, kh:kh + H:2, kw:kw + W:2][:, :H // 2, :W // 2]
            out = out + tap[..., None] * w64[:, 0, kh, kw]
    return out


# ------------------------------------------------------------------------------------------------ latent heads
def z_bound(ref_z, eps, lv64, bound_mu, bound_lv, u_out):
    """|z - (mu64 + eps exp(lv64 / 2))| for the kernel's z = round_T(mu + eps * expf(0.5f * lv)) computed from its own
    float32 mu / lv (within bound_mu / bound_lv of mu64 / lv64): the output rounding u_out |ref|, mu's error, and eps
    times the error of the standard deviation: d exp(lv / 2) = exp(lv / 2) * 0.5 * d lv, plus 4 float32 roundings
    (0.5f * lv, expf's own 2 ulp, the product with eps, the sum)."""
    return (u_out * ref_z.abs() + bound_mu +
            eps.abs() * torch.exp(0.5 * lv64) * (0.5 * bound_lv + 4 * 2.0 ** -23))


def elementwise_bound(ref64, absref64, k_terms, u_out):
    """The bound of exact_cases.assert_elementwise, as a tensor."""
    return u_out * ref64.abs() + (k_terms + 16) * 2.0 ** -23 * absref64


def ulp32(ref64):
    """Spacing of float32 at float32(ref64), as float64."""
    r = ref64.to(torch.float32).abs()
    return (torch.nextafter(r, torch.full_like(r, math.inf)) - r).to(F64)
