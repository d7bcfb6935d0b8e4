"""The float64 references of tests/bn_cases.py are torch's own arithmetic, not self-made truth: BatchNorm forward
against torch.nn.BatchNorm1d (train mode, running statistics and batch count included), the backward against autograd
through the same graph with a fixed dropout mask, the edge conv against F.conv2d, all within 1e-12 relative; and the
backward cases hold no element near the activation's kink."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as BC
from tests import exact_cases as X

RTOL = 1e-12
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def close(got, ref, what, scale=None):
    scale = scale or float(ref.abs().max()) or 1.0
    err = float((got - ref).abs().max())
    assert err <= RTOL * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def torch_act(z, act):
    return F.leaky_relu(z, 0.01) if act == 0 else F.relu(z) if act == 1 else z


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("R,C", [(255, 4), (3001, 32), (77, 1024), (2, 256), (5, 128)])
def test_forward_reference_is_torch_batchnorm(R, C, act):
    gen = torch.Generator().manual_seed(BC.seed_of(R, C, act))
    y = BC.quant(torch.randn(R, C, generator=gen) * 1.7 + 0.3, torch.bfloat16)
    gamma, beta, rm, rv = BC.bn_params(gen, C)
    mask = BC.make_mask(gen, R, C)
    bn = torch.nn.BatchNorm1d(C, eps=BC.f32(BC.EPS), momentum=BC.f32(BC.MOMENTUM)).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.train()
    ref1 = BC.bn_fwd_ref(y, gamma, beta, act, rm=rm, rv=rv)
    out = torch_act(bn(y), act).detach()
    close(ref1["a"], out, "a")
    close(ref1["rm"], bn.running_mean, "running_mean")
    close(ref1["rv"], bn.running_var, "running_var")
    assert int(bn.num_batches_tracked) == 1
    # the masked form and a second step on the blended statistics
    refm = BC.bn_fwd_ref(y, gamma, beta, act, mask=mask, mscale=BC.MSCALE)
    close(refm["a"], out * (mask != 0).double() * BC.f32(BC.MSCALE), "a masked")
    ref2 = BC.bn_fwd_ref(y, gamma, beta, act, rm=ref1["rm"], rv=ref1["rv"])
    bn(y)
    close(ref2["rm"], bn.running_mean, "running_mean, second step")
    close(ref2["rv"], bn.running_var, "running_var, second step")
    assert int(bn.num_batches_tracked) == 2
    # eval mode on those statistics
    bn.eval()
    rm2, rv2 = bn.running_mean.clone(), bn.running_var.clone()
    close(BC.bn_eval_ref(y, gamma, beta, act, rm2, rv2)["a"], torch_act(bn(y), act).detach(), "a eval")
    # the bound's magnitude dominates the value
    assert bool((ref1["absref"] >= ref1["a"].abs() * (1 - 1e-12)).all())


def test_forward_reference_single_row():
    """R == 1 (torch refuses it in train mode): variance 0, invstd 1 / sqrt(eps), the running variance blended with
    the biased value 0 (common.hpp bn_train_finalize)."""
    R, C = BC.FWD_R1
    gen = torch.Generator().manual_seed(1)
    y = torch.randn(R, C, generator=gen).double()
    gamma, beta, rm, rv = BC.bn_params(gen, C)
    ref = BC.bn_fwd_ref(y, gamma, beta, 0, rm=rm, rv=rv)
    assert bool((ref["var"] == 0).all())
    close(ref["invstd"], torch.full((C,), BC.f32(BC.EPS) ** -0.5, dtype=torch.float64), "invstd")
    close(ref["rv"], (1 - BC.f32(BC.MOMENTUM)) * rv.double(), "running_var")
    close(ref["a"], torch_act(beta.double(), 0).expand(R, C), "a")


def test_flat_layout_is_nchw_flatten():
    B, hw, C = 3, 6, 8
    a = torch.arange(B * hw * C, dtype=torch.float64).reshape(B * hw, C)
    nchw = a.reshape(B, 2, 3, C).permute(0, 3, 1, 2)
    assert torch.equal(BC.to_flat(a, hw), nchw.flatten(1))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C,act", [(64, 512, 1), (2, 256, 0), (5, 128, 2), (1500, 64, 0), (77, 1024, 1)])
@pytest.mark.parametrize("masked", [False, True])
def test_backward_reference_is_autograd(dt, R, C, act, masked):
    c = BC.bwd_case(dt, TDT[dt], R, C, act, masked)
    y = c["y"].clone().requires_grad_(True)
    gamma = c["gamma"].double().requires_grad_(True)
    beta = c["beta"].double().requires_grad_(True)
    a = torch_act(F.batch_norm(y, None, None, gamma, beta, training=True, eps=BC.f32(BC.EPS)), act)
    if masked:
        a = a * ((c["mask"] != 0).double() * BC.f32(BC.MSCALE))
    a.backward(c["da"])
    # the reference takes the statistics it is given: here the float64 ones, as autograd uses
    m, _, inv = BC.batch_stats(c["y"], BC.EPS)
    ref = BC.bn_bwd_ref(c["y"], c["da"], m, inv, c["gamma"], c["beta"], act, c["mask"], BC.MSCALE if masked else 1.0)
    # relative to the largest term of dy's three-term sum: at R = 2 they cancel to ~eps / var of their size
    g_inv = c["gamma"].double() * inv
    terms = g_inv * (ref["dz"].abs() + ref["dbeta"].abs() / R + ref["xhat"].abs() * ref["dgamma"].abs() / R)
    close(ref["dy"], y.grad, "dy", scale=float(terms.max()))
    close(ref["dgamma"], gamma.grad, "dgamma")
    close(ref["dbeta"], beta.grad, "dbeta")


def _all_bwd_cases():
    for dt in ("fp32", "bf16"):
        for R, C, act in BC.BWD_MASKED:
            yield dt, R, C, act, True
        for R, C, act in BC.BWD_SMALL:
            yield dt, R, C, act, False


def test_backward_cases_hold_no_element_near_the_kink():
    """Nothing is excluded from the GPU comparison: every case's y has no |z| < ZMIN after flip_free_y, also with
    the float32 statistics the kernel is given."""
    for dt, R, C, act, masked in _all_bwd_cases():
        c = BC.bwd_case(dt, TDT[dt], R, C, act, masked)
        assert BC.count_near_zero(c["y"], c["gamma"], c["beta"]) == 0, (dt, R, C, act)
        assert torch.equal(c["y"], BC.quant(c["y"], TDT[dt])) and torch.equal(c["da"], BC.quant(c["da"], TDT[dt]))
        z32 = (c["y"] - c["mean"].double()) * c["invstd"].double() * c["gamma"].double() + c["beta"].double()
        assert float(z32.abs().min()) > 0.5 * BC.ZMIN, (dt, R, C, act)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_edge_fused_ybn_holds_no_element_near_the_kink(dt):
    for B, Hi, Wi in BC.EDGE_FUSED:
        c = BC.edge_bn_case(TDT[dt], B, Hi, Wi)
        assert BC.count_near_zero(c["y"], c["gamma"], c["beta"]) == 0
        z32 = (c["y"] - c["mean"].double()) * c["invstd"].double() * c["gamma"].double() + c["beta"].double()
        assert float(z32.abs().min()) > 0.5 * BC.ZMIN


@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (3, 6, 10), (2, 16, 32)])
def test_edge_conv_reference_is_conv2d(B, H, W):
    gen = torch.Generator().manual_seed(BC.seed_of(B, H, W))
    x = torch.randn(B, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(32, 1, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(32, generator=gen, dtype=torch.float64)
    close(BC.conv_c1_plain(x, w, b), BC.conv_c1_ref(x, w, b), "conv_c1")
    assert BC.conv_c1_ref(x, w, b).shape == (B, H // 2, W // 2, 32)


def test_exact_forward_case_is_exact():
    """The exact-placement case: mean 0, invstd 0.5 and an integer z in float64, so every stored value is one float32
    product rounded once."""
    for dt in ("fp32", "bf16"):
        for R, C in BC.FWD_EXACT[dt]:
            gen = torch.Generator().manual_seed(BC.seed_of(R, C))
            y, gamma, beta = BC.exact_fwd_case(gen, R, C)
            m, var, inv = BC.batch_stats(y, 0.0)
            assert bool((m == 0).all()) and bool((var == 4).all()) and bool((inv == 0.5).all())
            assert bool((y.abs() == 2).all()) and bool((y.sum(0) == 0).all())
            for act in (1, 2):   # integers: exact in either dtype
                e = BC.exact_fwd_expected(y, gamma, beta, act, TDT[dt])
                assert torch.equal(e.double(), BC.bn_fwd_ref(y, gamma, beta, act, eps=0.0)["a"])
            e0 = BC.exact_fwd_expected(y, gamma, beta, 0, torch.float32).double()
            r0 = BC.bn_fwd_ref(y, gamma, beta, 0, eps=0.0)["a"]
            assert float((e0 - r0).abs().max()) <= 11 * 0.01 * 2.0 ** -23


def test_linear_split_plan_matches_the_documented_counts():
    """linear_splits restates gemm_ops.hip plan_nt; tests/exact_cases.py LINEAR documents its counts at N = 42."""
    assert [BC.linear_splits("bf16", 3, K, 42) for K in (384, 512, 896)] == [3, 4, 7]
    assert [BC.linear_splits("fp32", 3, K, 42) for K in (384, 512, 896)] == [6, 8, 14]
    for dt in ("fp32", "bf16"):
        s = [BC.linear_splits(dt, B, K, 2 * L) for B, K, L in BC.LATENT]
        assert min(s) == 1 and max(s) > 1, (dt, s)
        s = [BC.linear_splits(dt, B, K, L) for B, K, L in BC.LATENT]
        assert min(s) == 1 and max(s) > 1, (dt, s)


def test_latent_exact_cases_fit_the_budget():
    for B, K, L in BC.LATENT:
        X.check_budget(K, X.EXTRA_MAX)
    assert BC.ld8(6) == 16 and BC.ld8(10) == 24 and BC.ld8(16) == 24 and BC.ld8(32) == 40
