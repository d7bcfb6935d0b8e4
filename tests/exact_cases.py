"""Shape lists and comparison helpers shared by the op-level GEMM / conv tests (tests/test_ops_gpu.py: random data,
tests/test_ops_exact_gpu.py: integer data) and their CPU proof (tests/test_exact_cases_cpu.py).  No GPU imports.

Two checks sharper than a relative L2 norm over the whole tensor:

  * assert_exact: with small integer operands every product and every partial sum of an f32-accumulating kernel is an
    exact f32 value (|sum| < 2^24, exact_budget), whatever the tile shape, split-K count or summation order, so the
    output must equal the float64 reference bit for bit (a bf16 output: its one RNE rounding).  One dropped, doubled
    or misplaced term moves an element by at least 1.
  * assert_elementwise: with random data, every single element within
        |got - ref| <= u_out |ref| + (k_terms + 16) 2^-23 absref,
    absref = the same op on |operands| (with |bias| and |old|), u_out = 2^-8 (bf16: half an ulp, relative) or 2^-24
    (f32).  The second term is the standard K u bound of an f32 sum, doubled (the MFMA's rounding inside its 4- or
    8-term step is not specified)."""
import math

import torch

TWO24 = float(2 ** 24)
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}

# ------------------------------------------------------------------------------------------------ shape lists
# hlmc_op_conv_s2 (B, Hi, Wi, Ci, Co).  bf16 also covers the shapes of the LDS halo-tile kernels: Ci 32 -> Co 64 at
# Wi 64 and Ci 64 -> Co 128 at Wi 32; fp32 runs the gather GEMM at every shape.
CONV_S2 = [(2, 16, 16, 32, 64), (2, 8, 8, 64, 128), (3, 4, 4, 128, 256), (2, 4, 4, 256, 512), (2, 2, 2, 512, 512),
           (1, 8, 32, 32, 32), (5, 4, 8, 64, 64), (3, 16, 64, 32, 64), (2, 64, 64, 32, 64), (2, 32, 32, 64, 128),
           (3, 8, 32, 64, 128), (2, 16, 16, 128, 256), (3, 32, 16, 128, 256)]
# hlmc_op_subpixel (B, Hi, Wi, Ci, Co).  The Ci 64 -> Co 32, 32-wide and Ci 128 -> Co 64, 16-wide shapes run the LDS
# halo-tile kernels in bf16.
SUBPIXEL = [(2, 2, 2, 512, 512), (2, 4, 4, 512, 256), (2, 8, 8, 256, 128), (3, 16, 16, 128, 64), (2, 32, 32, 64, 32),
            (1, 2, 16, 512, 512), (2, 4, 4, 32, 64), (3, 8, 32, 64, 32), (2, 16, 16, 128, 64), (3, 8, 16, 128, 64),
            (2, 16, 8, 256, 128)]
# hlmc_op_wgrad_s2, conv orientation (B, Hl, Wl, M, C)
WGRAD_S2 = [(2, 8, 8, 64, 32), (2, 4, 4, 128, 64), (2, 2, 2, 512, 256), (3, 1, 1, 512, 512), (2, 16, 16, 32, 64),
            (4, 2, 8, 256, 128), (3, 8, 32, 64, 32), (1, 32, 32, 64, 32),
            # the conv-layout split-K reduces (plan_tn; G: the grouped reduce's groups)
            (8, 8, 8, 128, 128),    # bf16 S 2 / fp32 S 4: 16-byte conv reduce (C % 128)
            (16, 8, 8, 128, 128),   # bf16 S 4: 16-byte conv reduce; fp32 S 8: grouped, G 4
            (12, 8, 8, 64, 32),     # 96-wide; bf16 S 3: 4-byte conv reduce, tail; fp32 S 6: G 2
            (2, 4, 4, 16, 16)]      # S 1, C % 32 != 0: the grouped reduce's scattered store
# hlmc_op_wgrad_s2, ConvTranspose2d orientation (B, Hl, Wl, Ci, Co): L = X (low-res), Xh = dY (high-res)
WGRAD_S2_CONVT = (2, 4, 4, 128, 64)
# hlmc_op_linear (M, K, N, ldx, act, acc)
LINEAR = [(4, 768, 256, 768, 0, 0), (256, 2048, 1024, 2048, 0, 0), (5, 370, 128, 376, 1, 0),
          (256, 2314, 64, 2320, 0, 1), (33, 128, 1152, 136, 1, 0), (256, 74, 2304, 80, 0, 0),
          (2, 1024, 16384, 1152, 0, 0), (2, 1024, 16384, 1152, 0, 1),
          # N % 4 != 0: the scalar NT split-K reduce (plan_nt, one 64 x 64 tile)
          (3, 384, 42, 384, 0, 0),   # bf16 S 3: tail only; fp32 S 6: 4 + 2
          (3, 512, 42, 512, 0, 0),   # bf16 S 4: one group of 4, no tail; fp32 S 8
          (3, 896, 42, 896, 0, 1)]   # bf16 S 7: 4 + 3; fp32 S 14: 4 + 4 + 4 + 2
# hlmc_op_linear with relu_ref (M, K, N, acc)
LINEAR_RELU_MASK = [(256, 2048, 1024, 0), (256, 512, 512, 1), (4, 16384, 1024, 0), (3, 64, 40, 1)]
# hlmc_op_linear with bf16 inputs and an f32 output (out_f32 = 1: linear<bf16, float>) (M, K, N)
LINEAR_OUT_F32 = [(4, 768, 256), (3, 384, 42), (256, 2048, 1024)]
# hlmc_op_linear_wgrad (Mb, N, K)
LINEAR_WGRAD = [(4, 256, 768), (256, 1024, 2048), (32, 128, 370), (256, 64, 2314), (7, 2048, 1024),
                # the grouped TN reduce at both widths (8 columns: float4; 9 with the bias: scalar),
                # one 32 x 128 tile (plan_tn): S (G groups) fp32 / bf16
                (300, 8, 8),     # 2, ragged (1) / 1 (1)
                (512, 8, 8),     # 4 (2) / 2 (1)
                (1024, 8, 8),    # 8 (4) / 4 (2)
                (4096, 8, 8)]    # 32 (8) / 16 (4)
# the single-channel edge layers (B, H, W): the bench's 128 x 128 clip and a 128 x 1024 mel row band besides the small
# case; (16, 128, 128) gives the row-staged weight gradient (64-wide layers) two rows per block
EDGE_CONVS = [(3, 16, 32), (2, 128, 128), (2, 32, 64), (1, 16, 1024), (16, 128, 128)]
# hlmc_op_wgrad_c1 at odd low-res heights and B = 1 (B, Hl, Wl)
WGRAD_C1_ODD = [(1, 7, 64), (3, 11, 64), (1, 5, 64), (2, 9, 24)]

# The B = 256 layer shapes of the benchmarked step (bench.py: audio-only HybridVAE 128 x 128, bf16).  Encoder forward
# conv shapes = the decoder's data-gradient convs, decoder sub-pixel shapes = the encoder's data gradients, and the
# ten weight gradients reduce to five (Hl, Wl, M, C) shapes.
BB = 256
BENCH_CONV = [(64, 64, 32, 64), (32, 32, 64, 128), (16, 16, 128, 256), (8, 8, 256, 512), (4, 4, 512, 512)]
BENCH_SUBPIXEL = [(2, 2, 512, 512), (4, 4, 512, 256), (8, 8, 256, 128), (16, 16, 128, 64), (32, 32, 64, 32)]
BENCH_WGRAD = [(32, 32, 64, 32), (16, 16, 128, 64), (8, 8, 256, 128), (4, 4, 512, 256), (2, 2, 512, 512)]
# the four LDS halo-tile shapes of the bench step (kind 0 conv_s2 / 1 subpixel, Hi, Wi, Ci, Co)
HALO = [(0, 64, 64, 32, 64), (0, 32, 32, 64, 128), (1, 32, 32, 64, 32), (1, 16, 16, 128, 64)]
# Edge shapes of the same four layers (kind, B, Hi, Wi, Ci, Co): the persistent tile walk where it is not a whole
# number of equal passes.
#   minimal: B = 1 at the smallest legal height: fewer tiles than the grid cap (grid = tiles x channel splits), the
#     prefetch clamped on the block's only tile; the three one-tile shapes' tile is both first and last of its image
#     (zero row above / below, a_out ownership);
#   uneven: two tiles per image and two more tiles than a channel split has blocks (514 / 512, 130 / 128): two blocks
#     walk two tiles, the rest one.
HALO_EDGE = [(0, 1, 8, 64, 32, 64), (0, 1, 8, 32, 64, 128), (1, 1, 4, 32, 64, 32), (1, 1, 8, 16, 128, 64),
             (0, 257, 8, 64, 32, 64), (0, 65, 16, 32, 64, 128), (1, 257, 8, 32, 64, 32), (1, 65, 16, 16, 128, 64)]

# value ranges of the exact cases
OPERAND_MAX = 2   # operands in {-2..2}
EXTRA_MAX = 8     # bias and the accumulate's old values in {-8..8}


# ------------------------------------------------------------------------------------------------ exact data
def int_operands(gen, shape, lo=-OPERAND_MAX, hi=OPERAND_MAX):
    """Integer-valued float64 tensor, uniform over {lo..hi}."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(torch.float64)


def exact_budget(k_terms, amax, bmax, extra):
    """Worst-case |partial sum| of k_terms products of |a| <= amax, |b| <= bmax plus `extra` (|bias| + |old|).  Below
    2^24 every partial sum, in any order and any split, is an exact f32 value."""
    return float(k_terms) * float(amax) * float(bmax) + float(extra)


def check_budget(k_terms, extra=0, amax=OPERAND_MAX, bmax=OPERAND_MAX):
    budget = exact_budget(k_terms, amax, bmax, extra)
    assert budget < TWO24, f"integer case leaves the exact f32 range: |sum| up to {budget:g} >= 2^24"
    return budget


def exact_case_budgets():
    """(case name, exact_budget) of every shape the exact tests run, with their value ranges (operands {-2..2}, bias
    and old values {-8..8})."""
    a, e = OPERAND_MAX, EXTRA_MAX
    out = []
    for B, Hi, Wi, Ci, Co in CONV_S2:
        out.append((f"conv_s2 {(B, Hi, Wi, Ci, Co)}", exact_budget(9 * Ci, a, a, e)))
    for B, Hi, Wi, Ci, Co in SUBPIXEL:
        out.append((f"subpixel {(B, Hi, Wi, Ci, Co)}", exact_budget(9 * Ci, a, a, e)))
    for kind, B, Hi, Wi, Ci, Co in HALO_EDGE:
        out.append((f"halo edge {(kind, B, Hi, Wi, Ci, Co)}", exact_budget(9 * Ci, a, a, e)))
    for kind, Hi, Wi, Ci, Co in HALO:
        out.append((f"halo {(kind, BB, Hi, Wi, Ci, Co)}", exact_budget(9 * Ci, a, a, e)))
    for Hi, Wi, Ci, Co in BENCH_CONV + BENCH_SUBPIXEL:
        out.append((f"bench conv / subpixel {(BB, Hi, Wi, Ci, Co)}", exact_budget(9 * Ci, a, a, e)))
    for B, Hl, Wl, M, C in WGRAD_S2 + [WGRAD_S2_CONVT]:
        out.append((f"wgrad_s2 {(B, Hl, Wl, M, C)}", exact_budget(B * Hl * Wl, a, a, 0)))
    for Hl, Wl, M, C in BENCH_WGRAD:
        out.append((f"bench wgrad_s2 {(BB, Hl, Wl, M, C)}", exact_budget(BB * Hl * Wl, a, a, 0)))
    for M, K, N, ldx, act, acc in LINEAR:
        out.append((f"linear {(M, K, N)}", exact_budget(K, a, a, 2 * e)))
    for M, K, N, acc in LINEAR_RELU_MASK:
        out.append((f"linear relu mask {(M, K, N)}", exact_budget(K, a, a, e)))
    for M, K, N in LINEAR_OUT_F32:
        out.append((f"linear out_f32 {(M, K, N)}", exact_budget(K, a, a, 2 * e)))
    for Mb, N, K in LINEAR_WGRAD:
        out.append((f"linear_wgrad {(Mb, N, K)}", exact_budget(Mb, a, a, 0)))
    for B, H, W in EDGE_CONVS:
        out.append((f"conv_c1_s2 {(B, H, W)}", exact_budget(9, a, a, e)))
        out.append((f"convT_c1 {(B, H, W)}", exact_budget(9 * 32, a, a, e)))
        out.append((f"wgrad_c1 {(B, H, W)}", exact_budget(B * (H // 2) * (W // 2), a, a, 0)))
    for B, Hl, Wl in WGRAD_C1_ODD:
        out.append((f"wgrad_c1 odd {(B, Hl, Wl)}", exact_budget(B * Hl * Wl, a, a, 0)))
    return out


# ------------------------------------------------------------------------------------------------ guarded outputs
GUARD = 256


class Guarded:
    """An output tensor `t` with GUARD NaN elements before and after it; NaN-prefilled unless `init` is given."""

    def __init__(self, shape, dtype, device, init=None):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what):
        lo, hi = self.buf[:GUARD].isnan(), self.buf[-GUARD:].isnan()
        assert bool(lo.all()) and bool(hi.all()), (
            f"{what}: store outside the output: {int((~lo).sum())} guard elements before it "
            f"(offsets {(~lo).nonzero().reshape(-1)[:8].tolist()} of {GUARD}), {int((~hi).sum())} after it "
            f"(offsets {(~hi).nonzero().reshape(-1)[:8].tolist()})")


# ------------------------------------------------------------------------------------------------ comparisons
def _axes_for(ndim):
    return {4: ("b", "row", "col", "channel"), 2: ("row", "col"), 1: ("i",)}.get(ndim, tuple(f"d{i}" for i in range(ndim)))


def _coords(flat, shape, axes):
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return ", ".join(f"{a} {i}" for a, i in zip(axes, reversed(idx)))


def _tile_of(flat, shape, tile, gemm_cols):
    """Tile row / column of flat index `flat` in the GEMM view of the output: rows = the leading dimensions flattened,
    columns = the last `gemm_cols` dimensions flattened."""
    ncol = 1
    for n in shape[len(shape) - gemm_cols:]:
        ncol *= n
    r, c = flat // ncol, flat % ncol
    return (f"GEMM row {r} col {c} = tile ({r // tile[0]}, {c // tile[1]}) of {tile[0]} x {tile[1]}, "
            f"offset ({r % tile[0]}, {c % tile[1]})")


def mismatch_report(got, exp, what, tile=None, axes=None, gemm_cols=1):
    """Text that points at the wrong elements: how many, the first and the worst index in the op's own coordinates
    (and, with `tile` = (rows, cols), the GEMM tile they fall in), got and expected values."""
    g, e = got.detach().cpu().to(torch.float64).reshape(-1), exp.detach().cpu().to(torch.float64).reshape(-1)
    shape = tuple(exp.shape)
    axes = axes or _axes_for(len(shape))
    bad = ~((g == e) | (g.isnan() & e.isnan()))
    n_bad = int(bad.sum())
    if n_bad == 0:
        return f"{what}: no mismatching element"
    err = (g - e).abs()
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
    first = int(bad.nonzero()[0])
    worst = int(torch.where(bad, err, torch.full_like(err, -1.0)).argmax())
    lines = [f"{what}: {n_bad} of {g.numel()} elements differ (shape {shape})"]
    for name, i in (("first", first), ("worst", worst)):
        line = f"  {name}: [{_coords(i, shape, axes)}] got {float(g[i])!r} expected {float(e[i])!r}"
        if tile is not None:
            line += f"; {_tile_of(i, shape, tile, gemm_cols)}"
        lines.append(line)
    rows = bad.reshape(shape[0], -1).any(1).nonzero().reshape(-1)
    lines.append(f"  {axes[0]} indices with a mismatch: {rows[:16].tolist()}{' ...' if rows.numel() > 16 else ''}")
    return "\n".join(lines)


def assert_exact(got, ref64, out_dtype, what, tile=None, axes=None, gemm_cols=1):
    """got == ref64.to(out_dtype), element for element (compared on got's device; tensors come back only to report)."""
    assert got.dtype == out_dtype, (what, got.dtype, out_dtype)
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    exp = ref64.to(out_dtype)
    if torch.equal(got, exp.to(got.device)):
        return
    raise AssertionError(mismatch_report(got, exp, what, tile, axes, gemm_cols))


def assert_elementwise(got, ref64, absref64, k_terms, out_dtype, what):
    """Per element |got - ref| <= u_out |ref| + (k_terms + 16) 2^-23 absref.  Prints and returns the largest ratio of
    error to bound (0 where both are 0; inf where the bound is 0 and the error is not)."""
    assert got.dtype == out_dtype, (what, got.dtype, out_dtype)
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(absref64.shape), (what, got.shape, ref64.shape)
    dev = got.device
    ref, absref = ref64.to(dev, torch.float64), absref64.to(dev, torch.float64)
    err = (got.to(torch.float64) - ref).abs()
    bound = U_OUT[out_dtype] * ref.abs() + (k_terms + 16) * 2.0 ** -23 * absref
    ok = err <= bound                     # a NaN in got fails here
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: largest error / bound {worst:.3f} (k_terms {k_terms}, {str(out_dtype).replace('torch.', '')})")
    if not bool(ok.all()):
        n_bad = int((~ok).sum())
        i = int(ratio.reshape(-1).argmax())
        shape = tuple(ref64.shape)
        raise AssertionError(
            f"{what}: {n_bad} of {err.numel()} elements outside the per-element bound; worst at "
            f"[{_coords(i, shape, _axes_for(len(shape)))}]: got {float(got.reshape(-1)[i])!r} reference "
            f"{float(ref.reshape(-1)[i])!r} error {float(err.reshape(-1)[i]):.3e} bound "
            f"{float(bound.reshape(-1)[i]):.3e} (ratio {worst:.2f})")
    return worst
