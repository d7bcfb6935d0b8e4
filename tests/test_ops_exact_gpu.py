"""Exact-arithmetic parity of the HIP GEMM and conv ops: integer operands, zero tolerance (tests/exact_cases.py).

Both MFMA paths accumulate in f32 and the epilogues compute act(sum + bias) + old in f32 and round once (RNE), so with
operands in {-2..2}, bias and old values in {-8..8} every partial sum is an exact f32 value (|sum| < 2^24, asserted
per case) and the output must equal the CPU float64 reference bit for bit -- for any tile shape, split-K count, slab
order or prefetch depth.  One dropped, doubled or misplaced term moves an element by at least 1; the failure report
names the element and its GEMM tile.  Every output sits between two 256-element NaN guard bands that must stay NaN,
and starts as NaN itself unless the op accumulates into it (an element never stored stays NaN).

On an MI355X every case here is exact (181 cases, each well under a second).  The companion per-element check on
random data (assert_elementwise in tests/test_ops_gpu.py) reaches these largest error / bound ratios per family:
bf16 outputs 0.92 - 0.995 (conv_s2 0.974, subpixel 0.975, halo 0.973, linear 0.987, conv_c1_s2 0.995: the half-ulp
rounding term is tight), f32 outputs <= 0.093 (wgrad_s2 0.083, linear_wgrad 0.086, wgrad_c1 0.001, convT_c1 0.006);
the table is in that file's header."""
import pytest
import torch
import torch.nn.functional as F

import hlmc_amd  # noqa: F401  (loads the library)
from hlmc_amd import _lib as L
from tests import exact_cases as X
from tests.exact_cases import Guarded

pytestmark = pytest.mark.gpu
DT = {"fp32": (L.HLMC_F32, torch.float32), "bf16": (L.HLMC_BF16, torch.bfloat16)}
WS_BYTES = 512 << 20
PAD_POISON = 1000.0   # in the ldx / ldw / lddy padding columns: a read past K or N shows
NT_TILE, LINEAR_TILE, TN_TILE = (128, 64), (64, 64), (32, 128)   # the report's tile grid (gemm_ops.hip with_*_tile)
NAN = float("nan")


@pytest.fixture(scope="module")
def ws(cuda):
    return torch.empty(WS_BYTES, dtype=torch.uint8, device=cuda)


def seed_of(*dims):
    s = 0
    for d in dims:
        s = (s * 1009 + int(d)) % (2 ** 31 - 1)
    return s


def padded(t, ld):
    """[rows][ld] with t in the first columns and PAD_POISON in the padding."""
    out = torch.full((t.shape[0], ld), PAD_POISON, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ------------------------------------------------------------------------------------------------ conv / sub-pixel
_HALO_KEYS = {(k, X.BB, *s) for k, *s in X.HALO} | set(X.HALO_EDGE)
_conv_cache = {}


def conv_case(cuda, kind, dt, B, Hi, Wi, Ci, Co):
    """Device operands and the expected output (float64 reference rounded to the dtype) of conv_s2 (kind 0) /
    subpixel (1).  The halo-tile shapes are computed once: the plain op and hlmc_op_halo_fwd share them."""
    key = (kind, B, Hi, Wi, Ci, Co)
    if dt == "bf16" and key in _conv_cache:
        return _conv_cache[key]
    tdt = DT[dt][1]
    X.check_budget(9 * Ci, X.EXTRA_MAX)
    g = torch.Generator().manual_seed(seed_of(*key))
    x = X.int_operands(g, (B, Hi, Wi, Ci))
    b = X.int_operands(g, (Co,), -X.EXTRA_MAX, X.EXTRA_MAX)
    if kind == 0:
        w = X.int_operands(g, (Co, Ci, 3, 3))
        wp = w.permute(0, 2, 3, 1)
        ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1)
    else:
        w = X.int_operands(g, (Ci, Co, 3, 3))   # ConvTranspose2d weight layout -> [Co][kh][kw][Ci]
        wp = w.permute(1, 2, 3, 0)
        ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1, output_padding=1)
    ref = ref.permute(0, 2, 3, 1)
    assert float(ref.abs().max()) < X.TWO24
    out = (x.to(tdt).to(cuda).contiguous(), wp.contiguous().to(tdt).to(cuda), b.float().to(cuda),
           ref.to(tdt).contiguous().to(cuda))
    if dt == "bf16" and key in _HALO_KEYS:
        _conv_cache[key] = out
    return out


def run_conv(cuda, ws, kind, dt, B, Hi, Wi, Ci, Co):
    code, tdt = DT[dt]
    xd, wd, bd, exp = conv_case(cuda, kind, dt, B, Hi, Wi, Ci, Co)
    y = Guarded(tuple(exp.shape), tdt, cuda)
    op = L.lib().hlmc_op_conv_s2 if kind == 0 else L.lib().hlmc_op_subpixel
    L.check(op(L.stream(), code, xd.data_ptr(), B, Hi, Wi, Ci, wd.data_ptr(), bd.data_ptr(), Co, y.t.data_ptr(),
               ws.data_ptr(), WS_BYTES))
    torch.cuda.synchronize()
    what = f"{'conv_s2' if kind == 0 else 'subpixel'} {dt} B={B} {Hi}x{Wi} {Ci}->{Co}"
    X.assert_exact(y.t, exp, tdt, what, tile=NT_TILE)
    y.check(what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hi,Wi,Ci,Co", X.CONV_S2)
def test_conv_s2_exact(cuda, ws, dt, B, Hi, Wi, Ci, Co):
    run_conv(cuda, ws, 0, dt, B, Hi, Wi, Ci, Co)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hi,Wi,Ci,Co", X.SUBPIXEL)
def test_subpixel_exact(cuda, ws, dt, B, Hi, Wi, Ci, Co):
    run_conv(cuda, ws, 1, dt, B, Hi, Wi, Ci, Co)


@pytest.mark.parametrize("kind,B,Hi,Wi,Ci,Co", X.HALO_EDGE)
def test_halo_plain_edge_shapes_exact(cuda, ws, kind, B, Hi, Wi, Ci, Co):
    """hlmc_op_conv_s2 / hlmc_op_subpixel (bf16: the plain form of the LDS halo-tile kernels) where the persistent tile
    walk is not a whole number of equal passes."""
    run_conv(cuda, ws, kind, "bf16", B, Hi, Wi, Ci, Co)


@pytest.mark.parametrize("Hi,Wi,Ci,Co", X.BENCH_CONV)
def test_conv_s2_bench_shapes_exact(cuda, ws, Hi, Wi, Ci, Co):
    """B = 256: the split-K count, the <= 512-block LDS-DMA ring and the persistent tile walk depend on B."""
    run_conv(cuda, ws, 0, "bf16", X.BB, Hi, Wi, Ci, Co)


@pytest.mark.parametrize("Hi,Wi,Ci,Co", X.BENCH_SUBPIXEL)
def test_subpixel_bench_shapes_exact(cuda, ws, Hi, Wi, Ci, Co):
    run_conv(cuda, ws, 1, "bf16", X.BB, Hi, Wi, Ci, Co)


def _halo_fwd_exact(cuda, kind, B, Hi, Wi, Ci, Co):
    xd, wd, bd, exp = conv_case(cuda, kind, "bf16", B, Hi, Wi, Ci, Co)
    what = f"halo_fwd kind {kind} B={B} {Hi}x{Wi} {Ci}->{Co}"
    y = Guarded(tuple(exp.shape), torch.bfloat16, cuda)
    sums = Guarded((2 * Co,), torch.float64, cuda)
    g = torch.Generator().manual_seed(seed_of(kind, B, Hi, Ci))
    rm0, rv0 = torch.randn(Ci, generator=g), torch.rand(Ci, generator=g) + 0.5
    rm, rv = rm0.to(cuda), rv0.to(cuda)
    nbt = torch.full((1,), 7, dtype=torch.int64, device=cuda)
    mean_o, inv_o = torch.full((Ci,), NAN, device=cuda), torch.full((Ci,), NAN, device=cuda)
    a_out = Guarded((B, Hi, Wi, Ci), torch.bfloat16, cuda)
    wsb = int(L.lib().hlmc_op_halo_workspace(Ci, Co))
    hws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    P = L.ptr
    L.check(L.lib().hlmc_op_halo_fwd(L.stream(), kind, P(xd), B, Hi, Wi, Ci, P(wd), P(bd), Co, P(y.t), P(sums.t), None,
                                     None, P(rm), P(rv), P(nbt), 0.1, 1e-5, P(mean_o), P(inv_o), P(a_out.t), P(hws),
                                     wsb), "hlmc_op_halo_fwd")
    torch.cuda.synchronize()
    X.assert_exact(y.t, exp, torch.bfloat16, what, tile=NT_TILE)
    y.check(what)
    # the epilogue's statistics: integer sums and sums of squares of the stored bf16 output, both < 2^53, so exact in
    # float64 in any order
    e = exp.to(torch.float64).reshape(-1, Co)
    s_ref = torch.cat([e.sum(0), (e * e).sum(0)])
    assert float(s_ref.abs().max()) < 2.0 ** 53
    X.assert_exact(sums.t, s_ref, torch.float64, what + " out_sums (sum y | sum y^2)", axes=("column",))
    sums.check(what + " out_sums")
    # without gamma nothing of the input BatchNorm is touched
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt.item()) == 7
    assert bool(mean_o.isnan().all()) and bool(inv_o.isnan().all()) and bool(a_out.buf.isnan().all())


@pytest.mark.parametrize("kind,Hi,Wi,Ci,Co", X.HALO)
def test_halo_fwd_bench_shapes_exact(cuda, kind, Hi, Wi, Ci, Co):
    _halo_fwd_exact(cuda, kind, X.BB, Hi, Wi, Ci, Co)


@pytest.mark.parametrize("kind,B,Hi,Wi,Ci,Co", X.HALO_EDGE)
def test_halo_fwd_edge_shapes_exact(cuda, kind, B, Hi, Wi, Ci, Co):
    _halo_fwd_exact(cuda, kind, B, Hi, Wi, Ci, Co)


# ------------------------------------------------------------------------------------------------ conv weight gradients
def run_wgrad_s2(cuda, ws, dt, B, Hl, Wl, M, C, convT=False):
    """dW[M][C][3][3] = sum_{b,r,c} L[b,r,c,m] Xh[b,2r-1+kh,2c-1+kw,ci]; convT: L = the layer's low-res input
    (M = Ci), Xh = its output gradient (C = Co), reference through autograd of conv_transpose2d."""
    code, tdt = DT[dt]
    X.check_budget(B * Hl * Wl)
    g = torch.Generator().manual_seed(seed_of(B, Hl, Wl, M, C, int(convT)))
    lo = X.int_operands(g, (B, Hl, Wl, M))
    hi = X.int_operands(g, (B, 2 * Hl, 2 * Wl, C))
    if convT:
        w = torch.zeros(M, C, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(lo.permute(0, 3, 1, 2), w, stride=2, padding=1, output_padding=1).backward(
            hi.permute(0, 3, 1, 2))
        ref = w.grad
    else:
        ref = torch.nn.grad.conv2d_weight(hi.permute(0, 3, 1, 2), (M, C, 3, 3), lo.permute(0, 3, 1, 2), stride=2,
                                          padding=1)
    assert float(ref.abs().max()) < X.TWO24
    lod, hid = lo.to(tdt).to(cuda).contiguous(), hi.to(tdt).to(cuda).contiguous()
    dW = Guarded((M, C, 3, 3), torch.float32, cuda)
    L.check(L.lib().hlmc_op_wgrad_s2(L.stream(), code, lod.data_ptr(), B, Hl, Wl, M, hid.data_ptr(), C,
                                     dW.t.data_ptr(), ws.data_ptr(), WS_BYTES))
    torch.cuda.synchronize()
    what = f"wgrad_s2 {dt} B={B} {Hl}x{Wl} M={M} C={C}{' convT' if convT else ''}"
    # the GEMM's view: rows m, columns (kh, kw, ci)
    X.assert_exact(dW.t.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), torch.float32, what, tile=TN_TILE,
                   axes=("m", "kh", "kw", "c"), gemm_cols=3)
    dW.check(what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hl,Wl,M,C", X.WGRAD_S2)
def test_wgrad_s2_conv_exact(cuda, ws, dt, B, Hl, Wl, M, C):
    run_wgrad_s2(cuda, ws, dt, B, Hl, Wl, M, C)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_wgrad_s2_convT_exact(cuda, ws, dt):
    run_wgrad_s2(cuda, ws, dt, *X.WGRAD_S2_CONVT, convT=True)


@pytest.mark.parametrize("Hl,Wl,M,C", X.BENCH_WGRAD)
def test_wgrad_s2_bench_shapes_exact(cuda, ws, Hl, Wl, M, C):
    """B = 256: up to 342 split-K slabs and their grouped reduction; |sum| <= 262144 * 4."""
    run_wgrad_s2(cuda, ws, "bf16", X.BB, Hl, Wl, M, C)


# ------------------------------------------------------------------------------------------------ linear
def run_linear(cuda, ws, dt, M, K, N, ldx, act, acc, out_f32=0, mask=False, bias=True):
    code, tdt = DT[dt]
    odt = torch.float32 if out_f32 else tdt
    X.check_budget(K, 2 * X.EXTRA_MAX)
    g = torch.Generator().manual_seed(seed_of(M, K, N, ldx, act, acc, out_f32, int(mask)))
    x, w = X.int_operands(g, (M, K)), X.int_operands(g, (N, K))
    b = X.int_operands(g, (N,), -X.EXTRA_MAX, X.EXTRA_MAX)
    old = X.int_operands(g, (M, N), -X.EXTRA_MAX, X.EXTRA_MAX)
    relu = X.int_operands(g, (M, N), -1, 2).clamp_min(0)   # a post-ReLU activation: half the entries exactly 0
    ref = x @ w.T
    if bias:
        ref = ref + b
    if act:
        ref = ref.clamp_min(0)
    if acc:
        ref = ref + old
    if mask:
        ref = torch.where(relu > 0, ref, torch.zeros_like(ref))
    assert float(ref.abs().max()) < X.TWO24
    ldw = ((K + 7) // 8) * 8
    xd, wd = padded(x, ldx).to(tdt).to(cuda), padded(w, ldw).to(tdt).to(cuda)
    bd, rd = b.float().to(cuda), relu.to(odt).to(cuda)
    y = Guarded((M, N), odt, cuda, init=old.to(odt) if acc else None)
    L.check(L.lib().hlmc_op_linear(L.stream(), code, xd.data_ptr(), ldx, M, K, wd.data_ptr(), ldw,
                                   bd.data_ptr() if bias else None, N, y.t.data_ptr(), N, act, acc, out_f32,
                                   ws.data_ptr(), WS_BYTES, rd.data_ptr() if mask else None))
    torch.cuda.synchronize()
    what = (f"linear {dt}{' -> f32' if out_f32 else ''} M={M} K={K} N={N} ldx={ldx} ldw={ldw} act={act} acc={acc}"
            f"{' relu mask' if mask else ''}")
    X.assert_exact(y.t, ref, odt, what, tile=LINEAR_TILE)
    if mask:
        assert bool((y.t[rd <= 0] == 0).all()), what + ": non-zero where relu_ref <= 0"
    y.check(what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M,K,N,ldx,act,acc", X.LINEAR)
def test_linear_exact(cuda, ws, dt, M, K, N, ldx, act, acc):
    run_linear(cuda, ws, dt, M, K, N, ldx, act, acc)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M,K,N,acc", X.LINEAR_RELU_MASK)
def test_linear_relu_mask_exact(cuda, ws, dt, M, K, N, acc):
    run_linear(cuda, ws, dt, M, K, N, K, 0, acc, mask=True, bias=False)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("M,K,N", X.LINEAR_OUT_F32)
def test_linear_bf16_in_f32_out_exact(cuda, ws, M, K, N, acc):
    """out_f32 = 1 with bf16 inputs: the linear<bf16, float> instantiation (the engine's f32 heads)."""
    run_linear(cuda, ws, "bf16", M, K, N, K, 0, acc, out_f32=1)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Mb,N,K", X.LINEAR_WGRAD)
def test_linear_wgrad_exact(cuda, ws, dt, Mb, N, K):
    code, tdt = DT[dt]
    X.check_budget(Mb)
    g = torch.Generator().manual_seed(seed_of(Mb, N, K))
    dy, x = X.int_operands(g, (Mb, N)), X.int_operands(g, (Mb, K))
    ref, ref_b = dy.T @ x, dy.sum(0)
    ldd, ldx = ((N + 7) // 8) * 8, ((K + 7) // 8) * 8
    dyd, xd = padded(dy, ldd).to(tdt).to(cuda), padded(x, ldx).to(tdt).to(cuda)
    for with_bias in (False, True):  # the bias gradient through the GEMM's ones column, and without it
        dW = Guarded((N, K), torch.float32, cuda)
        db = Guarded((N,), torch.float32, cuda)
        L.check(L.lib().hlmc_op_linear_wgrad(L.stream(), code, dyd.data_ptr(), ldd, xd.data_ptr(), ldx, Mb, N, K,
                                             dW.t.data_ptr(), db.t.data_ptr() if with_bias else None, ws.data_ptr(),
                                             WS_BYTES))
        torch.cuda.synchronize()
        what = f"linear_wgrad {dt} Mb={Mb} N={N} K={K} db={with_bias}"
        X.assert_exact(dW.t, ref, torch.float32, what, tile=TN_TILE)
        dW.check(what)
        if with_bias:
            X.assert_exact(db.t, ref_b, torch.float32, what + " db")
            db.check(what + " db")
        else:
            assert bool(db.buf.isnan().all()), what + ": db written though NULL was passed"


# ------------------------------------------------------------------------------------------------ single-channel edge layers
def run_wgrad_c1(cuda, ws, dt, g, B, Hl, Wl, img, imgd):
    code, tdt = DT[dt]
    X.check_budget(B * Hl * Wl)
    dy = X.int_operands(g, (B, Hl, Wl, 32))
    ref = torch.nn.grad.conv2d_weight(img[:, None], (32, 1, 3, 3), dy.permute(0, 3, 1, 2), stride=2, padding=1)
    dyd = dy.to(tdt).to(cuda).contiguous()
    dW = Guarded((32, 1, 3, 3), torch.float32, cuda)
    L.check(L.lib().hlmc_op_wgrad_c1(L.stream(), code, dyd.data_ptr(), B, Hl, Wl, 32, imgd.data_ptr(), dW.t.data_ptr(),
                                     ws.data_ptr(), WS_BYTES))
    torch.cuda.synchronize()
    what = f"wgrad_c1 {dt} B={B} {Hl}x{Wl}"
    X.assert_exact(dW.t, ref, torch.float32, what, axes=("m", "c", "kh", "kw"))
    dW.check(what)


@pytest.mark.parametrize("shape", X.EDGE_CONVS)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_edge_convs_exact(cuda, ws, dt, shape):
    code, tdt = DT[dt]
    B, H, W = shape
    g = torch.Generator().manual_seed(seed_of(B, H, W))
    X.check_budget(9 * 32, X.EXTRA_MAX)
    # conv1 forward (f32 image and weight, output in dt)
    img, w1 = X.int_operands(g, (B, H, W)), X.int_operands(g, (32, 1, 3, 3))
    b1 = X.int_operands(g, (32,), -X.EXTRA_MAX, X.EXTRA_MAX)
    ref = F.conv2d(img[:, None], w1, b1, stride=2, padding=1).permute(0, 2, 3, 1)
    imgd, w1d, b1d = img.float().to(cuda), w1.float().to(cuda), b1.float().to(cuda)
    y = Guarded((B, H // 2, W // 2, 32), tdt, cuda)
    L.check(L.lib().hlmc_op_conv_c1_s2(L.stream(), code, imgd.data_ptr(), B, H, W, w1d.data_ptr(), b1d.data_ptr(), 32,
                                       y.t.data_ptr()))
    torch.cuda.synchronize()
    X.assert_exact(y.t, ref, tdt, f"conv_c1_s2 {dt} {shape}")
    y.check(f"conv_c1_s2 {dt} {shape}")
    # last convT (32 -> 1; input in dt, f32 weight and output)
    a, wT = X.int_operands(g, (B, H // 2, W // 2, 32)), X.int_operands(g, (32, 1, 3, 3))
    bT = X.int_operands(g, (1,), -X.EXTRA_MAX, X.EXTRA_MAX)
    refT = F.conv_transpose2d(a.permute(0, 3, 1, 2), wT, bT, stride=2, padding=1, output_padding=1)[:, 0]
    ad, wTd, bTd = a.to(tdt).to(cuda).contiguous(), wT.float().to(cuda), bT.float().to(cuda)
    out = Guarded((B, H, W), torch.float32, cuda)
    L.check(L.lib().hlmc_op_convT_c1(L.stream(), code, ad.data_ptr(), B, H // 2, W // 2, 32, wTd.data_ptr(),
                                     bTd.data_ptr(), out.t.data_ptr()))
    torch.cuda.synchronize()
    X.assert_exact(out.t, refT, torch.float32, f"convT_c1 {dt} {shape}", axes=("b", "row", "col"))
    out.check(f"convT_c1 {dt} {shape}")
    # weight gradient of conv1 (one-channel f32 high-res side)
    run_wgrad_c1(cuda, ws, dt, g, B, H // 2, W // 2, img, imgd)


@pytest.mark.parametrize("shape", X.WGRAD_C1_ODD)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_wgrad_c1_odd_heights_exact(cuda, ws, dt, shape):
    B, Hl, Wl = shape
    g = torch.Generator().manual_seed(seed_of(B, Hl, Wl))
    img = X.int_operands(g, (B, 2 * Hl, 2 * Wl))
    run_wgrad_c1(cuda, ws, dt, g, B, Hl, Wl, img, img.float().to(cuda))
