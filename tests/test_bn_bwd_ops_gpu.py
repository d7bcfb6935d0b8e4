"""Op-level parity of the BatchNorm backward variants hlmc_op_bn_bwd does not reach (it fixes LeakyReLU, no mask,
lda == C), through hlmc_op_bn_act_bwd: bn_bwd_moments_kernel<T, true> / bn_bwd_apply_kernel<T, true, *> (the dropout
mask of the dense layers, with the C > 512 finalize launch and its sums scratch), the act 1 / 2 instances of
bn_bwd_small_kernel, and a gradient row stride above C.  No case here takes bn_bwd_fused_kernel: with a mask the two
passes always run, without one R <= 1024 runs the small kernel.

Reference: float64 (tests/bn_cases.py bn_bwd_ref, pinned to autograd in tests/test_bn_cases_cpu.py) on operands that
hold no element near the activation's kink (flip_free_y), so nothing is excluded.  Tolerances are those of
test_bn_bwd_op_matches_reference: dy relative L2 1e-2 (bf16) / 1e-5 (fp32), the sums 1e-4 / 1e-5, dbias absolutely
against the stored dy's float64 column sums.

Measured on an MI355X, largest per family: dy relative L2 masked fp32 8.2e-8 / bf16 1.7e-3, small fp32 6.1e-7 / bf16
1.7e-3 (bf16: the output rounding); dgamma / dbeta 7.5e-8 at most; dbias error / bound 0.004 at most."""
import pytest
import torch

import hlmc_amd  # noqa: F401  (loads the library)
from hlmc_amd import _lib as L
from tests import bn_cases as BC
from tests.exact_cases import Guarded

pytestmark = pytest.mark.gpu
DT = {"fp32": (L.HLMC_F32, torch.float32), "bf16": (L.HLMC_BF16, torch.bfloat16)}
TOL = {"fp32": (1e-5, 1e-5), "bf16": (1e-2, 1e-4)}   # dy relative L2, dgamma / dbeta relative L2
P = L.ptr
HLMC_EINVAL = -1
RESULTS_MEASURED = {}   # family: [dy, sums, dbias error / bound], largest in this run (printed: pytest -s)


def rel(got, ref):
    g, r = got.detach().cpu().double(), ref.double()
    return float((g - r).norm() / r.norm().clamp_min(1e-300))


def run_bwd(cuda, dt, c, act, mscale, lda):
    """hlmc_op_bn_act_bwd on the case's operands; da with row stride lda (NaN in its padding columns)."""
    code, tdt = DT[dt]
    R, C = c["y"].shape
    da = torch.full((R, lda), float("nan"), dtype=tdt)
    da[:, :C] = c["da"].to(tdt)
    keep = [c["y"].to(cuda, tdt).contiguous(), da.to(cuda)] + [c[k].to(cuda) for k in ("mean", "invstd", "gamma", "beta")]
    mask = c["mask"].to(cuda).contiguous() if c["mask"] is not None else None
    o = {"dy": Guarded((R, C), tdt, cuda), "dgamma": Guarded((C,), torch.float32, cuda),
         "dbeta": Guarded((C,), torch.float32, cuda), "dbias": Guarded((C,), torch.float32, cuda)}
    wsb = int(L.lib().hlmc_op_bn_bwd_workspace(C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    L.check(L.lib().hlmc_op_bn_act_bwd(L.stream(), code, P(keep[1]), lda, P(keep[0]), R, C, P(keep[2]), P(keep[3]),
                                       P(keep[4]), P(keep[5]), act, P(mask), mscale, P(o["dy"].t), P(o["dgamma"].t),
                                       P(o["dbeta"].t), P(o["dbias"].t), P(ws), wsb), "hlmc_op_bn_act_bwd")
    torch.cuda.synchronize()
    L.check_device("hlmc_op_bn_act_bwd")
    return o


def check_bwd(dt, o, c, act, mscale, what, family):
    ref = BC.bn_bwd_ref(c["y"], c["da"], c["mean"], c["invstd"], c["gamma"], c["beta"], act, c["mask"], mscale)
    for k, g in o.items():
        g.check(f"{what} {k}")
        assert not bool(g.t.isnan().any()), f"{what}: {k} holds NaN (an element never stored, or a padding column read)"
    tol_dy, tol_s = TOL[dt]
    r_dy, r_g, r_b = rel(o["dy"].t, ref["dy"]), rel(o["dgamma"].t, ref["dgamma"]), rel(o["dbeta"].t, ref["dbeta"])
    dyh = o["dy"].t.double().cpu()
    err = (o["dbias"].t.cpu().double() - dyh.sum(0)).abs()
    bound = 1e-5 * dyh.abs().sum(0) + 1e-6
    r_bias = float((err / bound).max())
    print(f"{what}: dy {r_dy:.2e} / {tol_dy:g}, dgamma {r_g:.2e}, dbeta {r_b:.2e} / {tol_s:g}, "
          f"dbias error / bound {r_bias:.3f}")
    best = RESULTS_MEASURED.setdefault(family, [0.0, 0.0, 0.0])
    best[:] = [max(best[0], r_dy), max(best[1], r_g, r_b), max(best[2], r_bias)]
    print(f"largest so far, {family}: dy {best[0]:.2e}, sums {best[1]:.2e}, dbias error / bound {best[2]:.3f}")
    assert r_dy < tol_dy, f"{what}: dy relative L2 {r_dy:.3e}"
    assert r_g < tol_s and r_b < tol_s, f"{what}: dgamma {r_g:.3e} dbeta {r_b:.3e}"
    assert r_bias <= 1.0, f"{what}: dbias error / bound {r_bias:.3f}"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C,act", BC.BWD_MASKED)
@pytest.mark.parametrize("pad", [0, 16])
def test_bn_act_bwd_masked(cuda, dt, R, C, act, pad):
    """BatchNorm1d + activation + Dropout backward: the two-pass kernels' mask instances; C = 1024 runs the separate
    finalize launch with the sums scratch."""
    c = BC.bwd_case(dt, DT[dt][1], R, C, act, True)
    what = f"bn_act_bwd {dt} R={R} C={C} act={act} mask lda={C + pad}"
    o = run_bwd(cuda, dt, c, act, BC.MSCALE, C + pad)
    check_bwd(dt, o, c, act, BC.MSCALE, what, f"masked {dt}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C,act", BC.BWD_SMALL)
@pytest.mark.parametrize("pad", [0, 16])
def test_bn_act_bwd_small(cuda, dt, R, C, act, pad):
    """R <= 1024 without a mask: bn_bwd_small_kernel, <T, 0> for LeakyReLU and <T, -1> (runtime activation) else."""
    c = BC.bwd_case(dt, DT[dt][1], R, C, act, False)
    what = f"bn_act_bwd {dt} R={R} C={C} act={act} small lda={C + pad}"
    o = run_bwd(cuda, dt, c, act, 1.0, C + pad)
    check_bwd(dt, o, c, act, 1.0, what, f"small {dt}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bn_act_bwd_agrees_with_bn_bwd(cuda, dt):
    """act 0, no mask, lda == C is hlmc_op_bn_bwd's case: the two entries give the same bits (R <= 1024: the small
    kernel in both)."""
    code, tdt = DT[dt]
    R, C = 64, 512
    c = BC.bwd_case(dt, tdt, R, C, 0, False)
    o = run_bwd(cuda, dt, c, 0, 1.0, C)
    yd, dad = c["y"].to(cuda, tdt).contiguous(), c["da"].to(cuda, tdt).contiguous()
    st = [c[k].to(cuda) for k in ("mean", "invstd", "gamma", "beta")]
    dy = torch.empty(R, C, dtype=tdt, device=cuda)
    dg, db, dbias = (torch.empty(C, device=cuda) for _ in range(3))
    wsb = int(L.lib().hlmc_op_bn_bwd_workspace(C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    L.check(L.lib().hlmc_op_bn_bwd(L.stream(), code, P(dad), P(yd), R, C, P(st[0]), P(st[1]), P(st[2]), P(st[3]), P(dy),
                                   P(dg), P(db), P(dbias), P(ws), wsb))
    torch.cuda.synchronize()
    assert torch.equal(dy, o["dy"].t) and torch.equal(dg, o["dgamma"].t) and torch.equal(db, o["dbeta"].t)
    assert torch.equal(dbias, o["dbias"].t)


def test_bn_act_bwd_rejects_bad_arguments(cuda):
    R, C = 16, 64
    outs = {k: Guarded(s, torch.float32, cuda) for k, s in {"dy": (R, C), "dgamma": (C,), "dbeta": (C,),
                                                            "dbias": (C,)}.items()}
    x = torch.zeros(R, 2048, device=cuda)
    v = torch.ones(2048, device=cuda)
    wsb = int(L.lib().hlmc_op_bn_bwd_workspace(2048))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, da=P(x), lda=C, y=P(x), R=R, C=C, mean=P(v), dy=P(outs["dy"].t), dg=P(outs["dgamma"].t),
             act=0, ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_bn_act_bwd(L.stream(), dtype, da, lda, y, R, C, mean, P(v), P(v), P(v), act, None, 1.0,
                                          dy, dg, P(outs["dbeta"].t), P(outs["dbias"].t), ws_, wsb_)

    bad = {
        "da NULL": call(da=None), "y NULL": call(y=None), "mean NULL": call(mean=None), "dy NULL": call(dy=None),
        "dgamma NULL": call(dg=None), "ws NULL": call(ws_=None), "R 0": call(R=0), "R < 0": call(R=-1),
        "workspace too small": call(wsb_=int(L.lib().hlmc_op_bn_bwd_workspace(C)) - 1),
        "C 48 fp32": call(C=48, lda=48), "C 48 bf16": call(dtype=L.HLMC_BF16, C=48, lda=48),
        "C 4 bf16": call(dtype=L.HLMC_BF16, C=4, lda=8), "C 0": call(C=0),
        "lda not 16 bytes": call(lda=C + 2), "lda not 16 bytes bf16": call(dtype=L.HLMC_BF16, lda=C + 4),
        "lda < C": call(lda=C - 4), "act 3": call(act=3), "dtype 2": call(dtype=2),
    }
    torch.cuda.synchronize()
    wrong = {k: s for k, s in bad.items() if s != HLMC_EINVAL}
    assert not wrong, f"not rejected with HLMC_EINVAL: {wrong}"
    for k, g in outs.items():
        assert bool(g.buf.isnan().all()), f"{k} written by a rejected call"
    assert bool((ws == 0x5a).all()), "workspace written by a rejected call"
