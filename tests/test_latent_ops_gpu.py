"""Op-level parity of the latent reduces: linear_partials + heads_reparam (csrc/kernels.hip heads_reparam_kernel, the
kVec4 instantiation for L % 4 == 0 and the scalar one), linear_partials + reparam_bwd_reduce, and linear_wgrad_pair,
through hlmc_op_heads_reparam / hlmc_op_reparam_bwd_reduce / hlmc_op_linear_wgrad_pair.

  * mu / lv / gmu (d_mu NULL) / dW / db element by element against float64 (exact_cases.assert_elementwise, k_terms =
    the reduction length); with integer operands bit for bit at every split count;
  * S_out against the split plan restated in bn_cases.linear_splits (S > 1 and S == 1 both occur per dtype);
  * device noise: eps_keep bit-equal to hlmc_randn(seed, offset); z within bn_cases.z_bound of mu64 + eps exp(lv64 / 2);
  * gmu (d_mu NULL) bit-equal to hlmc_op_linear without bias: linear() and linear_partials() take the same plan
    (gemm_ops.hip with_linear_tile + nt_plan in both dispatch_linear and dispatch_linear_partials), the same register
    GEMM (pipe 0), and splitk_reduce_kernel's slab_sum<*, 1> (gemm.hpp) adds the slabs in ascending split order from
    0, as reparam_bwd_reduce_kernel does;
  * linear_wgrad_pair against float64 by the bound only: two hlmc_op_linear_wgrad calls on the column halves see
    M = N1 rows instead of 2 N1, and with_tn_tile / plan_tn (gemm_ops.hip) choose the tile and the split count from M,
    so the accumulation order differs.
Every output sits in a NaN-guarded buffer; the padding columns of z / gmu / glv must still be NaN afterwards.

Measured on an MI355X, largest error / bound per family (fp32 / bf16): mu and lv 0.003 / 0.001 (float32 outputs),
z 0.003 / 0.920, gmu 0.003 / 0.883, gmu and glv from the stored dz 0.309 / 0.995, the paired weight gradient 0.062 /
0.045; every integer case exact, gmu (d_mu NULL) bit-equal to hlmc_op_linear in all 18 cases."""
import ctypes

import pytest
import torch

import hlmc_amd  # noqa: F401  (loads the library)
from hlmc_amd import _lib as L
from tests import bn_cases as BC
from tests import exact_cases as X
from tests.exact_cases import Guarded

pytestmark = pytest.mark.gpu
DT = {"fp32": (L.HLMC_F32, torch.float32), "bf16": (L.HLMC_BF16, torch.bfloat16)}
P = L.ptr
SEED = 0x5EED1234ABCD
PAD_POISON = 1000.0
HLMC_EINVAL = -1
RATIOS_MEASURED = {}   # family: largest error / bound in this run (printed: pytest -s)
WGRAD_PAIR = [(B, K, Ln) for B, K, Ln in BC.LATENT] + [(300, 512, 16), (1024, 200, 6)]   # (Mb, K, N1)


def note(family, r):
    RATIOS_MEASURED[family] = max(RATIOS_MEASURED.get(family, 0.0), r)
    print(f"largest error / bound so far, {family}: {RATIOS_MEASURED[family]:.3f}")


def padded(t, ld, tdt, cuda):
    """[rows][ld] on the device with t in the first columns and PAD_POISON behind them."""
    out = torch.full((t.shape[0], ld), PAD_POISON, dtype=torch.float64)
    out[:, :t.shape[1]] = t
    return out.to(tdt).to(cuda)


def ceil8(n):
    return (n + 7) // 8 * 8


def workspace(cuda, dt, B, K, Ln):
    wsb = int(L.lib().hlmc_op_latent_workspace(DT[dt][0], B, K, Ln))
    return torch.empty(max(wsb, 16), dtype=torch.uint8, device=cuda), wsb


def within(got, ref64, bound64, what, family):
    err = (got.detach().cpu().double() - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound64)
    r = float(ratio.max())
    print(f"{what}: largest error / bound {r:.3f}")
    note(family, r)
    assert bool((err <= bound64).all()), f"{what}: error / bound {r:.3f} at flat index {int(ratio.argmax())}"


# ------------------------------------------------------------------------------------------------ heads + reparam
def heads_operands(dt, B, K, Ln, integer=False):
    tdt = DT[dt][1]
    gen = torch.Generator().manual_seed(BC.seed_of(B, K, Ln, int(integer)))
    if integer:
        X.check_budget(K, X.EXTRA_MAX)
        x, w = X.int_operands(gen, (B, K)), X.int_operands(gen, (2 * Ln, K))
        bias = X.int_operands(gen, (2 * Ln,), -X.EXTRA_MAX, X.EXTRA_MAX).float()
    else:
        x = BC.quant(torch.randn(B, K, generator=gen), tdt)
        w = BC.quant(torch.randn(2 * Ln, K, generator=gen) / K ** 0.5, tdt)
        bias = (0.1 * torch.randn(2 * Ln, generator=gen)).float()
    eps = torch.randn(B, Ln, generator=gen).float()
    full = x @ w.T + bias.double()
    absfull = x.abs() @ w.abs().T + bias.double().abs()
    return {"x": x, "w": w, "bias": bias, "eps": eps, "mu": full[:, :Ln], "lv": full[:, Ln:],
            "absmu": absfull[:, :Ln], "abslv": absfull[:, Ln:]}


def run_heads(cuda, dt, B, K, Ln, c, eps_in=None, offset=0, want_z=True, want_out=True):
    code, tdt = DT[dt]
    ldx, ldw, ldz = ceil8(K) + 8, ceil8(K), BC.ld8(Ln)
    xd, wd = padded(c["x"], ldx, tdt, cuda), padded(c["w"], ldw, tdt, cuda)
    bmu, blv = c["bias"][:Ln].contiguous().to(cuda), c["bias"][Ln:].contiguous().to(cuda)
    o = {k: Guarded((B, Ln), torch.float32, cuda) for k in ("mu", "lv", "mu_out", "lv_out", "eps_keep")}
    o["z"] = Guarded((B, ldz), tdt, cuda)
    ed = eps_in.to(cuda).contiguous() if eps_in is not None else None
    ws, wsb = workspace(cuda, dt, B, K, Ln)
    S = ctypes.c_int(-1)
    L.check(L.lib().hlmc_op_heads_reparam(
        L.stream(), code, P(xd), ldx, B, K, P(wd), ldw, Ln, P(bmu), P(blv), P(o["mu"].t), P(o["lv"].t),
        P(o["mu_out"].t) if want_out else None, P(o["lv_out"].t) if want_out else None, P(ed), SEED, offset,
        P(o["eps_keep"].t), P(o["z"].t) if want_z else None, ldz, ctypes.byref(S), P(ws), wsb), "hlmc_op_heads_reparam")
    torch.cuda.synchronize()
    o["S"] = S.value
    return o


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,K,Ln", BC.LATENT)
@pytest.mark.parametrize("variant", ["eps_in", "rng0", "rng4104", "encode", "no_out"])
def test_heads_reparam(cuda, dt, B, K, Ln, variant):
    tdt = DT[dt][1]
    c = heads_operands(dt, B, K, Ln)
    what = f"heads_reparam {dt} B={B} K={K} L={Ln} {variant}"
    rng = variant.startswith("rng")
    offset = 4104 if variant == "rng4104" else 0
    o = run_heads(cuda, dt, B, K, Ln, c, eps_in=None if rng else c["eps"], offset=offset, want_z=variant != "encode",
                  want_out=variant != "no_out")
    for k in ("mu", "lv", "mu_out", "lv_out", "eps_keep", "z"):
        o[k].check(f"{what} {k}")
    assert o["S"] == BC.linear_splits(dt, B, K, 2 * Ln), (what, o["S"])
    note(f"mu / lv {dt}", X.assert_elementwise(o["mu"].t, c["mu"], c["absmu"], K, torch.float32, what + " mu"))
    note(f"mu / lv {dt}", X.assert_elementwise(o["lv"].t, c["lv"], c["abslv"], K, torch.float32, what + " lv"))
    if variant == "no_out":
        assert bool(o["mu_out"].buf.isnan().all()) and bool(o["lv_out"].buf.isnan().all()), what + ": absent outputs"
    else:
        assert torch.equal(o["mu_out"].t, o["mu"].t) and torch.equal(o["lv_out"].t, o["lv"].t), what + ": copies"
    if variant == "encode":
        assert bool(o["eps_keep"].buf.isnan().all()) and bool(o["z"].buf.isnan().all()), what + ": encode only"
        return
    if rng:
        draw = Guarded((B * Ln,), torch.float32, cuda)
        L.check(L.lib().hlmc_randn(L.stream(), P(draw.t), B * Ln, SEED, offset))
        torch.cuda.synchronize()
        draw.check(what + " hlmc_randn")
        assert torch.equal(o["eps_keep"].t.reshape(-1), draw.t), what + ": eps_keep is not the stream's elements"
        assert bool(o["eps_keep"].t.isfinite().all()) and float(o["eps_keep"].t.abs().max()) < 7
    else:
        assert torch.equal(o["eps_keep"].t.cpu(), c["eps"]), what + ": eps_keep"
    eps = o["eps_keep"].t.cpu().double()
    zref = c["mu"] + eps * torch.exp(0.5 * c["lv"])
    u32 = X.U_OUT[torch.float32]
    bound = BC.z_bound(zref, eps, c["lv"], BC.elementwise_bound(c["mu"], c["absmu"], K, u32),
                       BC.elementwise_bound(c["lv"], c["abslv"], K, u32), X.U_OUT[tdt])
    within(o["z"].t[:, :Ln], zref, bound, what + " z", f"z {dt}")
    assert bool(o["z"].t[:, Ln:].isnan().all()), what + ": padding columns of z written"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,K,Ln", BC.LATENT)
def test_heads_reparam_exact(cuda, dt, B, K, Ln):
    """Integer operands: every partial sum is an exact float32, so mu / lv equal the float64 reference at any S."""
    c = heads_operands(dt, B, K, Ln, integer=True)
    what = f"heads_reparam exact {dt} B={B} K={K} L={Ln}"
    o = run_heads(cuda, dt, B, K, Ln, c, eps_in=c["eps"], want_z=False)
    X.assert_exact(o["mu"].t, c["mu"], torch.float32, what + " mu")
    X.assert_exact(o["lv"].t, c["lv"], torch.float32, what + " lv")
    X.assert_exact(o["mu_out"].t, c["mu"], torch.float32, what + " mu_out")
    for k in ("mu", "lv", "mu_out", "lv_out"):
        o[k].check(f"{what} {k}")


# ------------------------------------------------------------------------------------------------ reparam backward
def bwd_operands(dt, B, K, Ln, integer=False):
    tdt = DT[dt][1]
    gen = torch.Generator().manual_seed(BC.seed_of(B, K, Ln, 7, int(integer)))
    if integer:
        X.check_budget(K)
        x, w = X.int_operands(gen, (B, K)), X.int_operands(gen, (Ln, K))
    else:
        x = BC.quant(torch.randn(B, K, generator=gen), tdt)
        w = BC.quant(torch.randn(Ln, K, generator=gen) / K ** 0.5, tdt)
    f = lambda: torch.randn(B, Ln, generator=gen).float()   # noqa: E731
    return {"x": x, "w": w, "lv": 0.5 * f(), "eps": f(), "d_mu": f(), "d_lv": f(), "dz": x @ w.T,
            "absdz": x.abs() @ w.abs().T}


def run_bwd_reduce(cuda, dt, B, K, Ln, c, with_d):
    code, tdt = DT[dt]
    ldx, ldw, ldg = ceil8(K) + 8, ceil8(K), BC.ld8(Ln)
    xd, wd = padded(c["x"], ldx, tdt, cuda), padded(c["w"], ldw, tdt, cuda)
    f32s = {k: c[k].to(cuda).contiguous() for k in ("lv", "eps", "d_mu", "d_lv")}
    o = {"gmu": Guarded((B, ldg), tdt, cuda), "glv": Guarded((B, ldg), tdt, cuda)}
    ws, wsb = workspace(cuda, dt, B, K, Ln)
    S = ctypes.c_int(-1)
    L.check(L.lib().hlmc_op_reparam_bwd_reduce(
        L.stream(), code, P(xd), ldx, B, K, P(wd), ldw, Ln, P(f32s["lv"]), P(f32s["eps"]),
        P(f32s["d_mu"]) if with_d else None, P(f32s["d_lv"]) if with_d else None, P(o["gmu"].t), P(o["glv"].t), ldg,
        ctypes.byref(S), P(ws), wsb), "hlmc_op_reparam_bwd_reduce")
    torch.cuda.synchronize()
    o["S"], o["xd"], o["wd"], o["ldx"], o["ldw"] = S.value, xd, wd, ldx, ldw
    return o


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,K,Ln", BC.LATENT)
def test_reparam_bwd_reduce(cuda, dt, B, K, Ln):
    code, tdt = DT[dt]
    c = bwd_operands(dt, B, K, Ln)
    what = f"reparam_bwd_reduce {dt} B={B} K={K} L={Ln}"
    o0 = run_bwd_reduce(cuda, dt, B, K, Ln, c, with_d=False)
    o1 = run_bwd_reduce(cuda, dt, B, K, Ln, c, with_d=True)
    for o in (o0, o1):
        for k in ("gmu", "glv"):
            o[k].check(f"{what} {k}")
            assert bool(o[k].t[:, Ln:].isnan().all()), f"{what}: padding columns of {k} written"
        assert o["S"] == BC.linear_splits(dt, B, K, Ln), (what, o["S"])
    # d_mu NULL: gmu is the data gradient itself, a linear output
    gmu0 = o0["gmu"].t[:, :Ln]
    note(f"gmu {dt}", X.assert_elementwise(gmu0.contiguous(), c["dz"], c["absdz"], K, tdt, what + " gmu"))
    y = Guarded((B, Ln), tdt, cuda)
    lws = torch.empty(64 << 20, dtype=torch.uint8, device=cuda)
    L.check(L.lib().hlmc_op_linear(L.stream(), code, P(o0["xd"]), o0["ldx"], B, K, P(o0["wd"]), o0["ldw"], None, Ln,
                                   P(y.t), Ln, 0, 0, 0, P(lws), lws.numel(), None))
    torch.cuda.synchronize()
    y.check(what + " hlmc_op_linear")
    assert torch.equal(gmu0, y.t), what + ": gmu (d_mu NULL) differs from hlmc_op_linear"
    # the rest from the stored dz: six float32 roundings (0.5f * lv, expf within 2 ulp, three products, the sum), each
    # 2^-24 of the terms' magnitude, doubled as elsewhere: 8 * 2^-23; then the output rounding
    dzq = gmu0.double().cpu()
    lv, eps, u = c["lv"].double(), c["eps"].double(), X.U_OUT[tdt]
    term = dzq * eps * 0.5 * torch.exp(0.5 * lv)
    for o, dm, dl in ((o0, 0.0 * lv, 0.0 * lv), (o1, c["d_mu"].double(), c["d_lv"].double())):
        rmu, rlv = dm + dzq, dl + term
        within(o["gmu"].t[:, :Ln], rmu, u * rmu.abs() + 2.0 ** -23 * (dm.abs() + dzq.abs()), what + " gmu (stored dz)",
               f"gmu / glv from dz {dt}")
        within(o["glv"].t[:, :Ln], rlv, u * rlv.abs() + 8 * 2.0 ** -23 * (dl.abs() + term.abs()), what + " glv",
               f"gmu / glv from dz {dt}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("B,K,Ln", BC.LATENT)
def test_reparam_bwd_reduce_exact(cuda, dt, B, K, Ln):
    tdt = DT[dt][1]
    c = bwd_operands(dt, B, K, Ln, integer=True)
    o = run_bwd_reduce(cuda, dt, B, K, Ln, c, with_d=False)
    what = f"reparam_bwd_reduce exact {dt} B={B} K={K} L={Ln}"
    X.assert_exact(o["gmu"].t[:, :Ln].contiguous(), c["dz"], tdt, what + " gmu")
    o["gmu"].check(what)


# ------------------------------------------------------------------------------------------------ paired weight gradient
def run_wgrad_pair(cuda, dt, Mb, K, N1, integer):
    code, tdt = DT[dt]
    gen = torch.Generator().manual_seed(BC.seed_of(Mb, K, N1, 3, int(integer)))
    if integer:
        X.check_budget(Mb)
        dy, x = X.int_operands(gen, (Mb, 2 * N1)), X.int_operands(gen, (Mb, K))
    else:
        dy, x = BC.quant(torch.randn(Mb, 2 * N1, generator=gen), tdt), BC.quant(torch.randn(Mb, K, generator=gen), tdt)
    lddy, ldx = BC.ld8(2 * N1), ceil8(K) + 8
    dyd, xd = padded(dy, lddy, tdt, cuda), padded(x, ldx, tdt, cuda)
    o = {"dW1": Guarded((N1, K), torch.float32, cuda), "db1": Guarded((N1,), torch.float32, cuda),
         "dW2": Guarded((N1, K), torch.float32, cuda), "db2": Guarded((N1,), torch.float32, cuda)}
    ws, wsb = workspace(cuda, dt, Mb, K, N1)
    L.check(L.lib().hlmc_op_linear_wgrad_pair(L.stream(), code, P(dyd), lddy, P(xd), ldx, Mb, N1, K, P(o["dW1"].t),
                                              P(o["db1"].t), P(o["dW2"].t), P(o["db2"].t), P(ws), wsb),
            "hlmc_op_linear_wgrad_pair")
    torch.cuda.synchronize()
    ref = {"dW1": dy[:, :N1].T @ x, "db1": dy[:, :N1].sum(0), "dW2": dy[:, N1:].T @ x, "db2": dy[:, N1:].sum(0)}
    absref = {"dW1": dy[:, :N1].abs().T @ x.abs(), "db1": dy[:, :N1].abs().sum(0), "dW2": dy[:, N1:].abs().T @ x.abs(),
              "db2": dy[:, N1:].abs().sum(0)}
    return o, ref, absref


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Mb,K,N1", WGRAD_PAIR)
def test_linear_wgrad_pair(cuda, dt, Mb, K, N1):
    o, ref, absref = run_wgrad_pair(cuda, dt, Mb, K, N1, integer=False)
    what = f"linear_wgrad_pair {dt} Mb={Mb} K={K} N1={N1}"
    for k in ref:
        o[k].check(f"{what} {k}")
        note(f"wgrad pair {dt}", X.assert_elementwise(o[k].t, ref[k], absref[k], Mb, torch.float32, f"{what} {k}"))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("Mb,K,N1", WGRAD_PAIR)
def test_linear_wgrad_pair_exact(cuda, dt, Mb, K, N1):
    o, ref, _ = run_wgrad_pair(cuda, dt, Mb, K, N1, integer=True)
    what = f"linear_wgrad_pair exact {dt} Mb={Mb} K={K} N1={N1}"
    for k in ref:
        X.assert_exact(o[k].t, ref[k], torch.float32, f"{what} {k}")
        o[k].check(f"{what} {k}")


# ------------------------------------------------------------------------------------------------ bad arguments
def _rejected(bad, outs, ws):
    torch.cuda.synchronize()
    wrong = {k: s for k, s in bad.items() if s != HLMC_EINVAL}
    assert not wrong, f"not rejected with HLMC_EINVAL: {wrong}"
    for k, g in outs.items():
        assert bool(g.buf.isnan().all()), f"{k} written by a rejected call"
    assert bool((ws == 0x5a).all()), "workspace written by a rejected call"


def test_heads_reparam_rejects_bad_arguments(cuda):
    B, K, Ln = 3, 64, 8
    outs = {k: Guarded((B, 16), torch.float32, cuda) for k in ("mu", "lv", "eps_keep", "z")}
    x = torch.zeros(2 * Ln, K, device=cuda)
    wsb = int(L.lib().hlmc_op_latent_workspace(L.HLMC_F32, B, K, Ln))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, x_=P(x), ldx=K, B=B, K=K, w=P(x), ldw=K, Ln=Ln, bias=P(x), mu=P(outs["mu"].t), offset=0,
             keep=P(outs["eps_keep"].t), z=P(outs["z"].t), ldz=16, ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_heads_reparam(L.stream(), dtype, x_, ldx, B, K, w, ldw, Ln, bias, P(x), mu,
                                             P(outs["lv"].t), None, None, P(x), SEED, offset, keep, z, ldz, None, ws_,
                                             wsb_)

    _rejected({
        "x NULL": call(x_=None), "w NULL": call(w=None), "bias NULL": call(bias=None), "mu NULL": call(mu=None),
        "ws NULL": call(ws_=None), "B 0": call(B=0), "K 0": call(K=0), "L 0": call(Ln=0), "ldx < K": call(ldx=K - 8),
        "ldw < K": call(ldw=K - 8), "workspace too small": call(wsb_=wsb - 1), "offset % 4": call(offset=6),
        "z without eps_keep": call(keep=None), "ldz < L": call(ldz=4), "dtype 2": call(dtype=2),
    }, outs, ws)


def test_reparam_bwd_reduce_rejects_bad_arguments(cuda):
    B, K, Ln = 3, 64, 8
    outs = {k: Guarded((B, 16), torch.float32, cuda) for k in ("gmu", "glv")}
    x = torch.zeros(Ln, K, device=cuda)
    wsb = int(L.lib().hlmc_op_latent_workspace(L.HLMC_F32, B, K, Ln))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, x_=P(x), ldx=K, B=B, K=K, w=P(x), ldw=K, Ln=Ln, lv=P(x), eps=P(x), gmu=P(outs["gmu"].t),
             ldg=16, ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_reparam_bwd_reduce(L.stream(), dtype, x_, ldx, B, K, w, ldw, Ln, lv, eps, None, None, gmu,
                                                  P(outs["glv"].t), ldg, None, ws_, wsb_)

    _rejected({
        "x NULL": call(x_=None), "w NULL": call(w=None), "lv NULL": call(lv=None), "eps NULL": call(eps=None),
        "gmu NULL": call(gmu=None), "ws NULL": call(ws_=None), "B 0": call(B=0), "K -1": call(K=-1), "L 0": call(Ln=0),
        "ldx < K": call(ldx=K - 8), "workspace too small": call(wsb_=wsb - 1), "ldg < L": call(ldg=4),
        "dtype -1": call(dtype=-1),
    }, outs, ws)


def test_linear_wgrad_pair_rejects_bad_arguments(cuda):
    Mb, K, N1 = 5, 64, 8
    outs = {"dW1": Guarded((N1, K), torch.float32, cuda), "db1": Guarded((N1,), torch.float32, cuda),
            "dW2": Guarded((N1, K), torch.float32, cuda), "db2": Guarded((N1,), torch.float32, cuda)}
    x = torch.zeros(Mb, K, device=cuda)
    wsb = int(L.lib().hlmc_op_latent_workspace(L.HLMC_F32, Mb, K, N1))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, dy=P(x), lddy=2 * N1, x_=P(x), ldx=K, Mb=Mb, N1=N1, K=K, dW1=P(outs["dW1"].t),
             db2=P(outs["db2"].t), ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_linear_wgrad_pair(L.stream(), dtype, dy, lddy, x_, ldx, Mb, N1, K, dW1, P(outs["db1"].t),
                                                 P(outs["dW2"].t), db2, ws_, wsb_)

    _rejected({
        "dy NULL": call(dy=None), "x NULL": call(x_=None), "dW1 NULL": call(dW1=None), "db2 NULL": call(db2=None),
        "ws NULL": call(ws_=None), "Mb 0": call(Mb=0), "N1 0": call(N1=0), "K 0": call(K=0),
        "lddy < 2 N1": call(lddy=2 * N1 - 8), "ldx < K": call(ldx=K - 8), "workspace too small": call(wsb_=wsb - 1),
        "dtype 2": call(dtype=2),
    }, outs, ws)
