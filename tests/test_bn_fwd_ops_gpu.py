"""Op-level parity of the BatchNorm forward kernels (csrc/kernels.hip col_moments_kernel, bn_finalize_kernel,
bn_eval_kernel, bn_act_kernel in its mask / finalize / flat instances) through hlmc_op_bn_fwd, against the float64
references of tests/bn_cases.py (pinned to torch in tests/test_bn_cases_cpu.py).

Per case: the exact accumulator's column sums within the worst case of a float64 summation, R 2^-52 sum|term|; mean,
invstd and the running statistics within one float32 ulp of the float64 formula rounded to float32; the activation
element by element (exact_cases.assert_elementwise, k_terms 4); with the +-2 data of bn_cases.exact_fwd_case bit for
bit.  Every output sits in a NaN-guarded buffer and every padding column must still be NaN afterwards.

Measured on an MI355X (362 cases, the whole file under 5 s), largest error / bound of the activation per family:
bf16 train 0.995, masked 0.994, flat 0.993, eval 0.995 (the half-ulp output rounding is tight); fp32 train 0.082,
masked 0.074, flat 0.070, eval 0.090.  Every exact-placement case is exact, modes 0 / 1 / 2 agree bit for bit."""
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
NAN = float("nan")
HLMC_EINVAL = -1
RATIOS_MEASURED = {}   # family: largest error / bound ratio of `a` in this run (printed: pytest -s)


def run_fwd(cuda, dt, mode, y64, gamma, beta, act=0, mask=None, mscale=1.0, rm=None, rv=None, nbt=None, eps=BC.EPS,
            momentum=BC.MOMENTUM, lda=None, flat=None, state=None):
    """One hlmc_op_bn_fwd call.  `state` (a previous call's result) reuses its running buffers and count.  Returns the
    guarded outputs."""
    code, tdt = DT[dt]
    R, C = y64.shape
    dev = y64.device if y64.is_cuda else cuda
    yd = y64.to(dev, tdt).contiguous()
    o = {"R": R, "C": C, "tdt": tdt, "flat": flat, "keep": [yd]}
    o["mean"], o["invstd"] = Guarded((C,), torch.float32, cuda), Guarded((C,), torch.float32, cuda)
    o["sums"] = Guarded((2 * C,), torch.float64, cuda) if mode != 3 else None
    if state is not None:
        o["rm"], o["rv"], o["nbt"] = state["rm"], state["rv"], state["nbt"]
    else:
        o["rm"] = Guarded((C,), torch.float32, cuda, init=rm) if rm is not None else None
        o["rv"] = Guarded((C,), torch.float32, cuda, init=rv) if rv is not None else None
        o["nbt"] = torch.tensor([-7, nbt, -7], dtype=torch.int64, device=cuda) if nbt is not None else None
    if mode == 2:
        o["a"] = None
    elif flat:
        hw, ld = flat
        o["a"] = Guarded((R // hw, ld), tdt, cuda)
    else:
        o["a"] = Guarded((R, lda or C), tdt, cuda)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    md = mask.to(cuda).contiguous() if mask is not None else None
    wsb = int(L.lib().hlmc_op_bn_fwd_workspace(C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    o["keep"] += [gd, bd, md, ws]
    st = L.lib().hlmc_op_bn_fwd(
        L.stream(), code, mode, P(yd), R, C, P(gd), P(bd), act, P(md), mscale,
        P(o["rm"].t) if o["rm"] else None, P(o["rv"].t) if o["rv"] else None,
        o["nbt"][1:].data_ptr() if o["nbt"] is not None else None, momentum, eps, P(o["mean"].t), P(o["invstd"].t),
        P(o["a"].t) if o["a"] else None, lda or C, flat[0] if flat else 0, flat[1] if flat else 0,
        P(o["sums"].t) if o["sums"] else None, P(ws), wsb)
    L.check(st, "hlmc_op_bn_fwd")
    torch.cuda.synchronize()
    return o


def a_of(o):
    """The activation in [R][C] NHWC order and the padding columns."""
    R, C = o["R"], o["C"]
    t = o["a"].t
    if o["flat"]:
        hw, ld = o["flat"]
        body = t[:, :C * hw].reshape(R // hw, C, hw).permute(0, 2, 1).reshape(R, C)
        return body, t[:, C * hw:]
    return t[:, :C], t[:, C:]


def check_guards(o, what):
    for k in ("mean", "invstd", "sums", "rm", "rv", "a"):
        if o.get(k) is not None:
            o[k].check(f"{what} {k}")
    if o["a"] is not None:
        pad = a_of(o)[1]
        assert bool(pad.isnan().all()), f"{what}: {int((~pad.isnan()).sum())} padding elements of a written"
    if o["nbt"] is not None:
        assert o["nbt"][0].item() == -7 and o["nbt"][2].item() == -7, f"{what}: store next to num_batches_tracked"


def within_ulp(got, ref64, what, ulps=1):
    r32 = ref64.to(torch.float32).to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - r32).abs()
    ok = err <= ulps * BC.ulp32(ref64)
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {err.numel()} channels off by more than {ulps} float32 ulp; "
                            f"worst {float((err / BC.ulp32(ref64)).max()):.2f} ulp at channel "
                            f"{int((err / BC.ulp32(ref64)).argmax())}")


def check_sums(o, y64, what):
    y = y64.cpu()
    R = y.shape[0]
    ref = torch.cat([y.sum(0), (y * y).sum(0)])
    bound = R * 2.0 ** -52 * torch.cat([y.abs().sum(0), (y * y).sum(0)])
    err = (o["sums"].t.cpu() - ref).abs()
    assert bool((err <= bound).all()), f"{what} out_sums: worst error / bound {float((err / bound).max()):.2f}"


def check_stats(o, ref, what, count=None):
    within_ulp(o["mean"].t, ref["mean"], what + " mean")
    within_ulp(o["invstd"].t, ref["invstd"], what + " invstd")
    if o["rm"] is not None:
        within_ulp(o["rm"].t, ref["rm"], what + " running_mean")
        within_ulp(o["rv"].t, ref["rv"], what + " running_var")
    if count is not None:
        assert o["nbt"][1].item() == count, f"{what}: num_batches_tracked {o['nbt'][1].item()} != {count}"


def check_a(o, ref, family, what):
    body, _ = a_of(o)
    r = X.assert_elementwise(body, ref["a"], ref["absref"], 4, o["tdt"], what + " a")
    RATIOS_MEASURED[family] = max(RATIOS_MEASURED.get(family, 0.0), r)
    print(f"largest error / bound so far, {family}: {RATIOS_MEASURED[family]:.3f}")


def same_bits(o1, o2, what):
    for k in ("mean", "invstd", "sums", "rm", "rv", "a"):
        if o1.get(k) is not None and o2.get(k) is not None:
            a, b = o1[k].buf, o2[k].buf
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0), b.nan_to_num(0)), (
                f"{what}: {k} differs between the two modes")


def case(dt, R, C, *extra):
    tdt = DT[dt][1]
    gen = torch.Generator().manual_seed(BC.seed_of(R, C, *extra))
    y64 = BC.quant(torch.randn(R, C, generator=gen) * 1.7 + 0.3, tdt)
    gamma, beta, rm, rv = BC.bn_params(gen, C)
    return gen, y64, gamma, beta, rm, rv


# ------------------------------------------------------------------------------------------------ every shape, every mode
@pytest.mark.parametrize("dt,R,C", [(dt, R, C) for dt in ("fp32", "bf16") for R, C in BC.FWD_SHAPES[dt]])
def test_bn_fwd_shapes(cuda, dt, R, C):
    """Mode 0 (own moments pass) against the references; mode 1 (moments delivered) bit-identical to it in every
    output; mode 2 (bn_stats: moments + bn_finalize_kernel) bit-identical statistics; mode 3 (eval) on the blended
    running statistics."""
    _, y64, gamma, beta, rm, rv = case(dt, R, C)
    what = f"bn_fwd {dt} R={R} C={C}"
    ref = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    o0 = run_fwd(cuda, dt, 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    check_guards(o0, what)
    check_sums(o0, y64, what)
    check_stats(o0, ref, what, count=1)
    check_a(o0, ref, f"train {dt}", what)
    o1 = run_fwd(cuda, dt, 1, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    check_guards(o1, what + " mode 1")
    same_bits(o0, o1, what + " mode 0 / 1")
    assert o1["nbt"][1].item() == 1
    o2 = run_fwd(cuda, dt, 2, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    check_guards(o2, what + " mode 2")
    same_bits(o0, o2, what + " mode 0 / 2")
    assert o2["nbt"][1].item() == 1
    # eval on the running statistics mode 0 left: nothing but mean / invstd / a is written
    rm1, rv1 = o0["rm"].t.cpu(), o0["rv"].t.cpu()
    o3 = run_fwd(cuda, dt, 3, y64, gamma, beta, rm=rm1, rv=rv1, nbt=5)
    check_guards(o3, what + " eval")
    r3 = BC.bn_eval_ref(y64, gamma, beta, 0, rm1, rv1)
    assert torch.equal(o3["mean"].t.cpu(), rm1)
    # 1.f / sqrtf(rv + eps): three float32 roundings (the sum's halves through the root) stay below 1.25 ulp of the
    # result, plus the reference's own rounding
    within_ulp(o3["invstd"].t, r3["invstd"], what + " eval invstd", ulps=2)
    assert torch.equal(o3["rm"].t.cpu(), rm1) and torch.equal(o3["rv"].t.cpu(), rv1) and o3["nbt"][1].item() == 5
    check_a(o3, r3, f"eval {dt}", what + " eval")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bn_fwd_single_row(cuda, dt):
    """R = 1: variance 0, invstd 1 / sqrt(eps), the running variance blended with the biased value 0 (common.hpp
    bn_train_finalize), a = act(beta)."""
    R, C = BC.FWD_R1
    _, y64, gamma, beta, rm, rv = case(dt, R, C)
    what = f"bn_fwd {dt} R=1 C={C}"
    o = run_fwd(cuda, dt, 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    check_guards(o, what)
    ref = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    assert torch.equal(o["mean"].t.cpu().double(), y64[0])
    inv = torch.full((C,), BC.f32(BC.EPS) ** -0.5, dtype=torch.float64)
    within_ulp(o["invstd"].t, inv, what + " invstd")
    within_ulp(o["rv"].t, (1.0 - BC.f32(BC.MOMENTUM)) * rv.double(), what + " running_var")
    check_stats(o, ref, what, count=1)
    check_sums(o, y64, what)
    check_a(o, ref, f"train {dt}", what)


# ------------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C", BC.FWD_VARIANT_SHAPES)
@pytest.mark.parametrize("act", [1, 2])
def test_bn_fwd_activations(cuda, dt, R, C, act):
    _, y64, gamma, beta, rm, rv = case(dt, R, C)
    what = f"bn_fwd {dt} R={R} C={C} act={act}"
    ref = BC.bn_fwd_ref(y64, gamma, beta, act, rm=rm, rv=rv)
    o0 = run_fwd(cuda, dt, 0, y64, gamma, beta, act=act, rm=rm, rv=rv, nbt=0)
    check_guards(o0, what)
    check_stats(o0, ref, what, count=1)
    check_a(o0, ref, f"train {dt}", what)
    same_bits(o0, run_fwd(cuda, dt, 1, y64, gamma, beta, act=act, rm=rm, rv=rv, nbt=0), what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C", BC.FWD_VARIANT_SHAPES)
@pytest.mark.parametrize("pad", [0, 16])
def test_bn_fwd_masked(cuda, dt, R, C, pad):
    """BatchNorm1d + ReLU + Dropout: the mask is dense (stride C) while `a` has stride lda."""
    gen, y64, gamma, beta, rm, rv = case(dt, R, C)
    mask = BC.make_mask(gen, R, C)
    what = f"bn_fwd {dt} R={R} C={C} mask lda={C + pad}"
    ref = BC.bn_fwd_ref(y64, gamma, beta, 1, rm=rm, rv=rv, mask=mask, mscale=BC.MSCALE)
    o0 = run_fwd(cuda, dt, 0, y64, gamma, beta, act=1, mask=mask, mscale=BC.MSCALE, rm=rm, rv=rv, nbt=0, lda=C + pad)
    check_guards(o0, what)
    check_stats(o0, ref, what, count=1)
    check_a(o0, ref, f"masked {dt}", what)
    body = a_of(o0)[0]
    assert bool((body[(mask == 0).to(cuda)] == 0).all()), what + ": non-zero where the mask drops"
    o1 = run_fwd(cuda, dt, 1, y64, gamma, beta, act=1, mask=mask, mscale=BC.MSCALE, rm=rm, rv=rv, nbt=0, lda=C + pad)
    same_bits(o0, o1, what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("C", BC.FWD_FLAT_C)
@pytest.mark.parametrize("hw,B", BC.FWD_FLAT)
def test_bn_fwd_flat_output(cuda, dt, C, hw, B):
    """The NCHW-flat store (FlatOut) of the encoder's last activation: [B][C * hw + 8]."""
    R = B * hw
    _, y64, gamma, beta, rm, rv = case(dt, R, C, hw)
    what = f"bn_fwd {dt} R={B}*{hw} C={C} flat"
    ref = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    o0 = run_fwd(cuda, dt, 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0, flat=(hw, C * hw + 8))
    check_guards(o0, what)
    check_stats(o0, ref, what, count=1)
    check_a(o0, ref, f"flat {dt}", what)
    # the layout itself, against the NHWC output of the same call
    on = run_fwd(cuda, dt, 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    assert torch.equal(o0["a"].t[:, :C * hw], BC.to_flat(on["a"].t, hw)), what + ": flat order"
    same_bits(o0, run_fwd(cuda, dt, 1, y64, gamma, beta, rm=rm, rv=rv, nbt=0, flat=(hw, C * hw + 8)), what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("R,C", BC.FWD_VARIANT_SHAPES)
def test_bn_fwd_running_statistics(cuda, dt, R, C):
    """Absent running statistics leave everything else unchanged; two successive calls on the same buffers count
    0 -> 1 -> 2 and blend twice."""
    _, y64, gamma, beta, rm, rv = case(dt, R, C)
    what = f"bn_fwd {dt} R={R} C={C}"
    ref1 = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    o_none = run_fwd(cuda, dt, 0, y64, gamma, beta)
    check_guards(o_none, what + " no running")
    o1 = run_fwd(cuda, dt, 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    same_bits(o_none, o1, what + " with / without running statistics")
    check_stats(o1, ref1, what + " first call", count=1)
    rm1, rv1 = o1["rm"].t.cpu(), o1["rv"].t.cpu()
    y2 = BC.quant(y64 * 0.5 - 1.0, DT[dt][1])
    o2 = run_fwd(cuda, dt, 0, y2, gamma, beta, state=o1)
    check_guards(o2, what + " second call")
    ref2 = BC.bn_fwd_ref(y2, gamma, beta, 0, rm=rm1, rv=rv1)   # blended from the stored float32 values
    check_stats(o2, ref2, what + " second call", count=2)
    # and from the start, in float64 throughout: the first call's rounding to float32 (half an ulp of that value,
    # within one ulp as checked above) comes through the blend scaled by 1 - momentum, then the second call's own ulp
    ref2b = BC.bn_fwd_ref(y2, gamma, beta, 0, rm=ref1["rm"], rv=ref1["rv"])
    for k, name in (("rm", "running_mean"), ("rv", "running_var")):
        err = (o2[k].t.cpu().double() - ref2b[k].float().double()).abs()
        bound = BC.ulp32(ref2b[k]) + (1.0 - BC.f32(BC.MOMENTUM)) * BC.ulp32(ref1[k])
        assert bool((err <= bound).all()), f"{what} {name} after two calls: error / bound {float((err / bound).max()):.2f}"


# ------------------------------------------------------------------------------------------------ exact placement
def _flat_hw(R):
    return next(h for h in (6, 4, 2) if R % h == 0)


@pytest.mark.parametrize("dt,R,C", [(dt, R, C) for dt in ("fp32", "bf16") for R, C in BC.FWD_EXACT[dt]])
@pytest.mark.parametrize("variant", ["plain", "mask", "lda", "flat"])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_fwd_exact_placement(cuda, dt, R, C, variant, act):
    """+-2 in every column, eps 0, gamma a power of two, integer beta: mean 0, invstd 0.5 and every stored value one
    exactly reproducible float32 product.  A row or column stored in the wrong place, dropped or doubled changes a
    sign or a scale."""
    tdt = DT[dt][1]
    gen = torch.Generator().manual_seed(BC.seed_of(R, C))
    y64, gamma, beta = BC.exact_fwd_case(gen, R, C)
    mask = BC.make_mask(gen, R, C) if variant == "mask" else None
    mscale = BC.MSCALE if mask is not None else 1.0
    kw = {}
    if variant in ("mask", "lda"):
        kw["lda"] = C + 16
    if variant == "flat":
        hw = _flat_hw(R)
        kw["flat"] = (hw, C * hw + 8)
    what = f"bn_fwd exact {dt} R={R} C={C} act={act} {variant}"
    rm, rv = torch.zeros(C), torch.ones(C)
    exp = BC.exact_fwd_expected(y64, gamma, beta, act, tdt, mask, BC.f32(mscale))
    for mode in (0, 1):
        o = run_fwd(cuda, dt, mode, y64, gamma, beta, act=act, mask=mask, mscale=mscale, rm=rm, rv=rv, nbt=0, eps=0.0,
                    **kw)
        check_guards(o, what)
        assert bool((o["mean"].t == 0).all()) and bool((o["invstd"].t == 0.5).all()), what + ": mean 0, invstd 0.5"
        sums = torch.cat([torch.zeros(C), torch.full((C,), 4.0 * R)]).double()
        X.assert_exact(o["sums"].t, sums, torch.float64, what + " out_sums", axes=("column",))
        X.assert_exact(a_of(o)[0].contiguous(), exp.double(), tdt, what + " a", axes=("row", "channel"))
        within_ulp(o["rm"].t, torch.zeros(C, dtype=torch.float64), what + " running_mean")
        within_ulp(o["rv"].t, (1 - BC.f32(BC.MOMENTUM)) + BC.f32(BC.MOMENTUM) * 4.0 * R / (R - 1) *
                   torch.ones(C, dtype=torch.float64), what + " running_var")


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bn_fwd_nonfinite_columns(cuda, dt):
    """One NaN in column 3, one +inf in column 5: those columns' mean, invstd, running statistics and activation are
    NaN; every other column is untouched by them."""
    R, C, cn, ci = BC.NONFINITE
    _, y64, gamma, beta, rm, rv = case(dt, R, C)
    ref = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    ybad = y64.clone()
    ybad[1234, cn] = NAN
    ybad[77, ci] = float("inf")
    what = f"bn_fwd {dt} non-finite"
    for mode in (0, 1):
        o = run_fwd(cuda, dt, mode, ybad, gamma, beta, rm=rm, rv=rv, nbt=0)
        check_guards(o, what)
        good = torch.ones(C, dtype=torch.bool)
        good[[cn, ci]] = False
        body = a_of(o)[0]
        for k in ("mean", "invstd", "rm", "rv"):
            v = o[k].t.cpu()
            assert bool(v[~good].isnan().all()), f"{what}: {k} of the non-finite columns {v[~good].tolist()}"
            assert bool(v[good].isfinite().all()), f"{what}: {k} of another column is not finite"
        assert bool(body[:, ~good].isnan().all()), what + ": a of the non-finite columns"
        s = o["sums"].t.cpu()
        assert bool(s[[cn, C + cn, ci, C + ci]].isnan().all()) and bool(s[torch.cat([good, good])].isfinite().all())
        sub = {k: ref[k][..., good] for k in ("mean", "invstd", "rm", "rv", "a", "absref")}
        within_ulp(o["mean"].t.cpu()[good], sub["mean"], what + " mean")
        within_ulp(o["invstd"].t.cpu()[good], sub["invstd"], what + " invstd")
        within_ulp(o["rm"].t.cpu()[good], sub["rm"], what + " running_mean")
        within_ulp(o["rv"].t.cpu()[good], sub["rv"], what + " running_var")
        X.assert_elementwise(body[:, good.to(cuda)].contiguous(), sub["a"], sub["absref"], 4, DT[dt][1], what + " a")


# ------------------------------------------------------------------------------------------------ grid-stride loop
def test_bn_fwd_grid_stride_second_pass(cuda):
    """The only large case: bn_act_kernel's grid is capped at 8192 blocks of rpp * kU rows (256 * 4 at C = 4 fp32), so
    the second iteration of its grid-stride loop is not reached below 8192 * 1024 rows = 33.5 M elements.  The
    reference is computed in float64 on the device."""
    R, C = BC.FWD_GRID_STRIDE
    gen = torch.Generator(device=cuda).manual_seed(11)
    y64 = (torch.randn(R, C, generator=gen, device=cuda) * 1.7 + 0.3).double()
    gamma, beta, rm, rv = (t.to(cuda) for t in BC.bn_params(torch.Generator().manual_seed(12), C))
    what = f"bn_fwd fp32 R={R} C={C}"
    o = run_fwd(cuda, "fp32", 0, y64, gamma, beta, rm=rm, rv=rv, nbt=0)
    check_guards(o, what)
    ref = BC.bn_fwd_ref(y64, gamma, beta, 0, rm=rm, rv=rv)
    check_stats(o, {k: v.cpu() for k, v in ref.items() if k in ("mean", "invstd", "rm", "rv")}, what, count=1)
    check_a(o, ref, "train fp32", what)
    last = o["a"].t[-3:].isnan().any().item()
    assert not last, what + ": the last rows were not written"


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bn_fwd_rejects_bad_arguments(cuda):
    """Every rejected call returns HLMC_EINVAL without a launch: the outputs keep their NaN prefill."""
    R, C = 16, 64
    outs = {k: Guarded(s, d, cuda) for k, (s, d) in {
        "a": ((R, C + 16), torch.float32), "mean": ((C,), torch.float32), "invstd": ((C,), torch.float32),
        "sums": ((2 * C,), torch.float64), "rm": ((C,), torch.float32), "rv": ((C,), torch.float32)}.items()}
    y = torch.zeros(R, 2048, device=cuda)
    gb = torch.ones(2048, device=cuda)
    mask = torch.ones(R, C, dtype=torch.uint8, device=cuda)
    wsb = int(L.lib().hlmc_op_bn_fwd_workspace(2048))
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device=cuda)

    def call(dtype=L.HLMC_F32, mode=0, y=P(y), R=R, C=C, gamma=P(gb), a=P(outs["a"].t), lda=C, mask=None, rm=None,
             rv=None, mean=P(outs["mean"].t), hw=0, ld=0, sums=P(outs["sums"].t), ws_=P(ws), wsb_=wsb):
        return L.lib().hlmc_op_bn_fwd(L.stream(), dtype, mode, y, R, C, gamma, P(gb), 0, mask, 1.0, rm, rv, None, 0.1,
                                      1e-5, mean, P(outs["invstd"].t), a, lda, hw, ld, sums, ws_, wsb_)

    bad = {
        "y NULL": call(y=None), "gamma NULL": call(gamma=None), "a NULL": call(a=None), "mean NULL": call(mean=None),
        "ws NULL": call(ws_=None), "R 0": call(R=0), "R < 0": call(R=-3),
        "workspace too small": call(wsb_=int(L.lib().hlmc_op_bn_fwd_workspace(C)) - 1),
        "C 48 fp32": call(C=48, lda=48), "C 48 bf16": call(dtype=L.HLMC_BF16, C=48, lda=48),
        "C 4 bf16": call(dtype=L.HLMC_BF16, C=4, lda=8), "C 2048 fp32": call(C=2048, lda=2048), "C 0": call(C=0),
        "lda not 16 bytes": call(lda=C + 2), "lda not 16 bytes bf16": call(dtype=L.HLMC_BF16, lda=C + 4),
        "lda < C": call(lda=C - 4),
        "flat with a mask": call(mask=P(mask), hw=4, ld=C * 4), "flat ld too small": call(hw=4, ld=C * 4 - 4),
        "flat R % hw": call(hw=3, ld=C * 3),
        "running_mean alone": call(rm=P(outs["rm"].t)), "eval without running statistics": call(mode=3, sums=None),
        "eval with out_sums": call(mode=3, rm=P(outs["rm"].t), rv=P(outs["rv"].t)),
        "mode 4": call(mode=4), "dtype 2": call(dtype=2),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in bad.items() if v != HLMC_EINVAL}
    assert not wrong, f"not rejected with HLMC_EINVAL: {wrong}"
    for k, g in outs.items():
        assert bool(g.buf.isnan().all()), f"{k} written by a rejected call"
    assert bool((ws == 0x5a).all()), "workspace written by a rejected call"
    assert L.lib().hlmc_last_error().decode().startswith("hlmc_op_bn_fwd")
