"""Op-level parity of the statistics-fused forms of the single-channel edge conv (csrc/kernels.hip
conv_c1_s2_kernel<T, 32, 1> and <T, 32, 2>) through hlmc_op_conv_c1_s2_fused, and of the BnBwdFuse hand-over into
bn_act_bwd's apply pass.

  * y is bit-identical to hlmc_op_conv_c1_s2 (MODE 0 of the same template, pinned exactly by test_edge_convs_exact);
  * mode 1: out_sums against the float64 sums of the stored y and y^2; mode 2: against the float64 sums of dz and
    dz xhat, dz = y_stored lrelu'(xhat gamma + beta); per column |err| <= 1e-5 sum|term| + 1e-6, the project's form
    for per-thread float32 accumulation (a thread accumulates at most 8 pixels at these shapes: 8 x 2^-24 of sum|term|
    is the derived worst case, 1e-5 leaves a margin of 20);
  * mode 2 + bn_act_bwd(fused): dy / dgamma / dbeta against the float64 reference with the tolerances of
    tests/test_bn_bwd_ops_gpu.py, and dy against hlmc_op_bn_act_bwd on the stored gradient (its own moments pass);
  * integer data: mode 1's sums are exact integers.
C = 32 never takes the one-launch spin kernel (xacc_shards(32) = 16 > kBnFusedShards).

Measured on an MI355X, largest error / bound of out_sums: mode 1 fp32 0.0035, bf16 0.00003; mode 2 fp32 0.0031, bf16
0.0027.  Hand-over: dy relative L2 fp32 5.2e-8, bf16 1.7e-3; dgamma / dbeta 6.3e-8 at most; fused against unfused dy
fp32 1.1e-8, bf16 7.0e-7.  At R = 1 (one output pixel) the reference dy is exactly 0, a relative error has no meaning
and the test bounds |dy| absolutely instead (see there): |dy| / bound 0.10 fp32, 0.09 bf16."""
import pytest
import torch

import hlmc_amd  # noqa: F401  (loads the library)
from hlmc_amd import _lib as L
from tests import bn_cases as BC
from tests import exact_cases as X
from tests.exact_cases import Guarded

pytestmark = pytest.mark.gpu
DT = {"fp32": (L.HLMC_F32, torch.float32), "bf16": (L.HLMC_BF16, torch.bfloat16)}
TOL = {"fp32": (1e-5, 1e-5), "bf16": (1e-2, 1e-4)}
P = L.ptr
CO = 32
HLMC_EINVAL = -1
RATIOS_MEASURED = {}   # family: largest in this run (printed: pytest -s)


def rel(got, ref):
    g, r = got.detach().cpu().double(), ref.double()
    return float((g - r).norm() / r.norm().clamp_min(1e-300))


def note(family, r):
    RATIOS_MEASURED[family] = max(RATIOS_MEASURED.get(family, 0.0), r)
    print(f"largest so far, {family}: {RATIOS_MEASURED[family]:.3e}")


def conv_operands(cuda, B, Hi, Wi, integer=False):
    gen = torch.Generator().manual_seed(BC.seed_of(B, Hi, Wi, int(integer)))
    if integer:
        x, w = X.int_operands(gen, (B, Hi, Wi)), X.int_operands(gen, (CO, 1, 3, 3))
        b = X.int_operands(gen, (CO,), -X.EXTRA_MAX, X.EXTRA_MAX)
    else:
        x = torch.randn(B, Hi, Wi, generator=gen).double()
        w = 0.3 * torch.randn(CO, 1, 3, 3, generator=gen).double()
        b = 0.1 * torch.randn(CO, generator=gen).double()
    return x, w, b, x.float().to(cuda), w.float().to(cuda), b.float().to(cuda)


def plain_conv(cuda, dt, xd, wd, bd, B, Hi, Wi):
    code, tdt = DT[dt]
    y = Guarded((B, Hi // 2, Wi // 2, CO), tdt, cuda)
    L.check(L.lib().hlmc_op_conv_c1_s2(L.stream(), code, P(xd), B, Hi, Wi, P(wd), P(bd), CO, P(y.t)))
    torch.cuda.synchronize()
    return y


def fused(cuda, dt, mode, xd, wd, bd, B, Hi, Wi, bn=None, apply=False):
    code, tdt = DT[dt]
    R = B * (Hi // 2) * (Wi // 2)
    o = {"y": Guarded((B, Hi // 2, Wi // 2, CO), tdt, cuda), "sums": Guarded((2 * CO,), torch.float64, cuda)}
    keep = []
    args = [None] * 5
    if bn is not None:
        keep = [bn["y"].to(cuda, tdt).contiguous()] + [bn[k].to(cuda) for k in ("mean", "invstd", "gamma", "beta")]
        args = [P(t) for t in keep]
    if apply:
        o["dy"] = Guarded((R, CO), tdt, cuda)
        o["dgamma"], o["dbeta"] = Guarded((CO,), torch.float32, cuda), Guarded((CO,), torch.float32, cuda)
    wsb = int(L.lib().hlmc_op_conv_c1_s2_fused_workspace(CO))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    L.check(L.lib().hlmc_op_conv_c1_s2_fused(
        L.stream(), code, mode, P(xd), B, Hi, Wi, P(wd), P(bd), CO, P(o["y"].t), P(o["sums"].t), *args,
        P(o["dy"].t) if apply else None, P(o["dgamma"].t) if apply else None, P(o["dbeta"].t) if apply else None,
        P(ws), wsb), "hlmc_op_conv_c1_s2_fused")
    torch.cuda.synchronize()
    L.check_device("hlmc_op_conv_c1_s2_fused")
    return o


def check_sums(o, ref, absref, what, family):
    err = (o["sums"].t.cpu() - ref).abs()
    bound = 1e-5 * absref + 1e-6
    r = float((err / bound).max())
    print(f"{what} out_sums: largest error / bound {r:.3f}")
    note(family, r)
    assert r <= 1.0, f"{what} out_sums: error / bound {r:.3f} at column {int((err / bound).argmax())}"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hi,Wi", BC.EDGE_FUSED)
def test_conv_c1_s2_forward_statistics(cuda, dt, B, Hi, Wi):
    """MODE 1: the conv with the BatchNorm statistics of its stored output."""
    _, _, _, xd, wd, bd = conv_operands(cuda, B, Hi, Wi)
    what = f"conv_c1_s2 mode 1 {dt} {(B, Hi, Wi)}"
    y0 = plain_conv(cuda, dt, xd, wd, bd, B, Hi, Wi)
    o = fused(cuda, dt, 1, xd, wd, bd, B, Hi, Wi)
    for k, g in o.items():
        g.check(f"{what} {k}")
    assert torch.equal(o["y"].t, y0.t), what + ": y differs from hlmc_op_conv_c1_s2"
    ys = o["y"].t.double().cpu().reshape(-1, CO)
    check_sums(o, torch.cat([ys.sum(0), (ys * ys).sum(0)]), torch.cat([ys.abs().sum(0), (ys * ys).sum(0)]), what,
               f"mode 1 sums {dt}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hi,Wi", BC.EDGE_FUSED)
def test_conv_c1_s2_backward_moments_and_handover(cuda, dt, B, Hi, Wi):
    """MODE 2: the conv as a data gradient with the BatchNorm backward moments of its output, then bn_act_bwd's apply
    pass alone on those moments (BnBwdFuse::done)."""
    code, tdt = DT[dt]
    _, _, _, xd, wd, bd = conv_operands(cuda, B, Hi, Wi)
    bn = BC.edge_bn_case(tdt, B, Hi, Wi)
    R = bn["y"].shape[0]
    what = f"conv_c1_s2 mode 2 {dt} {(B, Hi, Wi)}"
    y0 = plain_conv(cuda, dt, xd, wd, bd, B, Hi, Wi)
    om = fused(cuda, dt, 2, xd, wd, bd, B, Hi, Wi, bn=bn)            # moments only
    o = fused(cuda, dt, 2, xd, wd, bd, B, Hi, Wi, bn=bn, apply=True)
    for k, g in list(o.items()) + list(om.items()):
        g.check(f"{what} {k}")
    assert torch.equal(o["y"].t, y0.t) and torch.equal(om["y"].t, y0.t), what + ": y differs from hlmc_op_conv_c1_s2"
    assert torch.equal(o["sums"].t, om["sums"].t), what + ": the apply pass changed the moments"
    da = y0.t.double().cpu().reshape(R, CO)                          # the stored gradient
    ref = BC.bn_bwd_ref(bn["y"], da, bn["mean"], bn["invstd"], bn["gamma"], bn["beta"], 0)
    dz, xh = ref["dz"], ref["xhat"]
    check_sums(o, torch.cat([dz.sum(0), (dz * xh).sum(0)]), torch.cat([dz.abs().sum(0), (dz * xh).abs().sum(0)]), what,
               f"mode 2 sums {dt}")
    # the hand-over
    tol_dy, tol_s = TOL[dt]
    assert not bool(o["dy"].t.isnan().any())
    r_g, r_b = rel(o["dgamma"].t, ref["dgamma"]), rel(o["dbeta"].t, ref["dbeta"])
    note(f"hand-over sums {dt}", max(r_g, r_b))
    assert r_g < tol_s and r_b < tol_s, (what, r_g, r_b)
    cancels = float(ref["dy"].norm()) == 0.0
    if cancels:
        # R == 1: xhat is 0 and dz - sum dz / R cancels exactly, so the reference is 0 and a relative error has no
        # meaning.  The kernel's float32 evaluation of that sum (three terms, each rounded once, the products free to
        # contract into the subtraction) leaves at most 4 x 2^-24 of the terms' magnitude, times gamma invstd.
        assert R == 1
        g_inv = (bn["gamma"].double() * bn["invstd"].double()).abs()
        terms = g_inv * (dz.abs() + ref["dbeta"].abs() / R + xh.abs() * ref["dgamma"].abs() / R)
        dy_bound = 4 * 2.0 ** -24 * terms
        r_dy = float((o["dy"].t.double().cpu().abs() / dy_bound).max())
        print(f"{what}: reference dy is 0; |dy| / bound {r_dy:.3f}")
        note(f"hand-over |dy| / bound at R = 1 {dt}", r_dy)
        assert r_dy <= 1.0, (what, r_dy)
    else:
        r_dy = rel(o["dy"].t, ref["dy"])
        print(f"{what}: dy {r_dy:.2e} / {tol_dy:g}, dgamma {r_g:.2e}, dbeta {r_b:.2e} / {tol_s:g}")
        note(f"hand-over dy {dt}", r_dy)
        assert r_dy < tol_dy, (what, r_dy)
    # against the unfused backward on the stored gradient (its own moments pass: other per-thread partial sums, so
    # not the same bits)
    keep = [bn["y"].to(cuda, tdt).contiguous()] + [bn[k].to(cuda) for k in ("mean", "invstd", "gamma", "beta")]
    dy2 = Guarded((R, CO), tdt, cuda)
    dg2, db2 = Guarded((CO,), torch.float32, cuda), Guarded((CO,), torch.float32, cuda)
    wsb = int(L.lib().hlmc_op_bn_bwd_workspace(CO))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    L.check(L.lib().hlmc_op_bn_act_bwd(L.stream(), code, P(y0.t), CO, P(keep[0]), R, CO, P(keep[1]), P(keep[2]),
                                       P(keep[3]), P(keep[4]), 0, None, 1.0, P(dy2.t), P(dg2.t), P(db2.t), None, P(ws),
                                       wsb), "hlmc_op_bn_act_bwd")
    torch.cuda.synchronize()
    dy2.check(what + " unfused dy")
    if cancels:
        assert bool((dy2.t.double().cpu().abs() <= dy_bound).all()), what + ": unfused dy at R = 1"
    else:
        r2 = rel(o["dy"].t, dy2.t.double().cpu())
        print(f"{what}: dy fused against unfused {r2:.2e}")
        note(f"hand-over dy fused / unfused {dt}", r2)
        assert r2 < tol_dy, (what, r2)
    assert rel(o["dgamma"].t, dg2.t.double().cpu()) < tol_s and rel(o["dbeta"].t, db2.t.double().cpu()) < tol_s


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Hi,Wi", BC.EDGE_FUSED)
def test_conv_c1_s2_forward_statistics_exact(cuda, dt, B, Hi, Wi):
    """Integer image, weights and bias: y and the sums of y and y^2 are small integers (per thread below 2^24, the block
    tree and the accumulator exact), so out_sums equals the integer totals bit for bit."""
    tdt = DT[dt][1]
    X.check_budget(9, X.EXTRA_MAX)
    x, w, b, xd, wd, bd = conv_operands(cuda, B, Hi, Wi, integer=True)
    what = f"conv_c1_s2 mode 1 exact {dt} {(B, Hi, Wi)}"
    ref = BC.conv_c1_ref(x, w, b)
    o = fused(cuda, dt, 1, xd, wd, bd, B, Hi, Wi)
    for k, g in o.items():
        g.check(f"{what} {k}")
    X.assert_exact(o["y"].t, ref, tdt, what)
    r = ref.reshape(-1, CO)
    # a thread's float32 partial sums stay exact: at most 8 pixels of y^2 <= (9 * 4 + 8)^2
    assert 8 * float((r * r).max()) < X.TWO24
    X.assert_exact(o["sums"].t, torch.cat([r.sum(0), (r * r).sum(0)]), torch.float64, what + " out_sums",
                   axes=("column",))


def test_conv_c1_s2_fused_rejects_bad_arguments(cuda):
    B, Hi, Wi = 1, 4, 4
    outs = {"y": Guarded((B, 2, 2, CO), torch.float32, cuda), "sums": Guarded((2 * CO,), torch.float64, cuda),
            "dy": Guarded((4, CO), torch.float32, cuda), "dgamma": Guarded((CO,), torch.float32, cuda),
            "dbeta": Guarded((CO,), torch.float32, cuda)}
    x = torch.zeros(B, Hi, Wi, device=cuda)
    v = torch.ones(4 * CO * 9, device=cuda)
    wsb = int(L.lib().hlmc_op_conv_c1_s2_fused_workspace(CO))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, mode=1, x=P(x), B=B, Hi=Hi, Wi=Wi, w=P(v), Co=CO, y=P(outs["y"].t),
             sums=P(outs["sums"].t), ybn=None, mean=None, dy=None, dg=None, ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_conv_c1_s2_fused(L.stream(), dtype, mode, x, B, Hi, Wi, w, P(v), Co, y, sums, ybn, mean,
                                                P(v), P(v), P(v), dy, dg, P(outs["dbeta"].t), ws_, wsb_)

    bad = {
        "x NULL": call(x=None), "w NULL": call(w=None), "y NULL": call(y=None), "out_sums NULL": call(sums=None),
        "ws NULL": call(ws_=None), "B 0": call(B=0), "odd H": call(Hi=3), "W 0": call(Wi=0), "Co 64": call(Co=64),
        "Co 48": call(Co=48), "workspace too small": call(wsb_=wsb - 1), "mode 0": call(mode=0), "mode 3": call(mode=3),
        "dtype 2": call(dtype=2), "mode 2 without ybn": call(mode=2, mean=P(v)),
        "mode 2 without mean": call(mode=2, ybn=P(v)),
        "dy_out without dgamma": call(mode=2, ybn=P(v), mean=P(v), dy=P(outs["dy"].t)),
    }
    torch.cuda.synchronize()
    wrong = {k: s for k, s in bad.items() if s != HLMC_EINVAL}
    assert not wrong, f"not rejected with HLMC_EINVAL: {wrong}"
    for k, g in outs.items():
        assert bool(g.buf.isnan().all()), f"{k} written by a rejected call"
    assert bool((ws == 0x5a).all()), "workspace written by a rejected call"
